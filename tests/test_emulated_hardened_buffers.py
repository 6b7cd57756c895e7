"""Poisoned and guarded device buffers (tests/test_gpu_hardened_buffers.py) and k_sweep_wide on the emulated device: a named subset,
byte comparisons with the oracle, run in a child process against tests/emu/_build/libspiral_emu.so (SPIRAL_HIP_LIB), as
tests/test_emulated_narrow_batch.py runs its file.  Plain build: poison_ws and guard_ws are the library's own instruments (a byte
fill at allocation, guard regions compared at release) and need no sanitizer."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emulated_library as emu_build  # noqa: E402
from test_emulated_library import _run  # noqa: E402

FILE = "test_gpu_hardened_buffers.py"
# both checks that the instruments work: a fresh partial buffer reads the poison, a byte written into a front guard is reported
INSTRUMENTS = "test_poison_reaches_a_fresh_partial_buffer or test_guard_reports_a_write_before_the_partial_buffer"
# a single query on the narrow FAST56 database, on the PACKED 64 x 128 one and on the same shape's 8-byte words (k_sweep_wide); the
# narrow and the sparse group lists: every one on buffers filled with 0xA5 and between guard regions
FLOWS = ("(single-fast56 or single-packed or single-db-unpacked or list5-fast56-narrow-group or list5-and-1-sparse-bucket) "
         "and (poison-a5 or guard)")
# every stage export, sp_multiply_reg_by_database at (64, 4), (300, 128) and (5, 128) among them
EXPORTS = "stage-exports and (poison-a5 or guard)"
# the new wide export shapes with at most 5 rows (tests/test_gpu_parity.py): one row, and three rows of two 128-column chunks
WIDE_SHAPES = "test_multiply_reg_by_database_shapes and (odd-1-128 or odd-3-256)"


@pytest.fixture(scope="module")
def emulated():
    so = emu_build.build()
    if so is None:
        pytest.skip("no host clang to build the emulated library with")
    return so


def test_instruments_work_on_the_emulated_device(emulated):
    assert _run(emulated, INSTRUMENTS, at_least=2, test_file=FILE) >= 2


def test_flows_on_poisoned_and_guarded_buffers_on_the_emulated_device(emulated):
    assert _run(emulated, FLOWS, at_least=10, test_file=FILE) >= 10


def test_stage_exports_on_poisoned_and_guarded_buffers_on_the_emulated_device(emulated):
    assert _run(emulated, EXPORTS, at_least=2, test_file=FILE) >= 2


def test_wide_sweep_small_shapes_on_the_emulated_device(emulated):
    assert _run(emulated, WIDE_SHAPES, at_least=2) >= 2
