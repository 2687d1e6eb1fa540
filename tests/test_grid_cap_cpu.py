"""SPRK_FE_MAX_GRID without a device: ``sprk_segments_grid(items)`` is the grid every capped launch of the ratings pipelines and the trainers
takes (csrc/host_segments.h fe_grid_capped).  Unset, it is what it was before the switch existed -- ceil(items / 256) up to 2048 -- so every
launch is; set to an integer in [1, 2048] it is capped there; anything else is ignored.  tests/test_gpu_grid_rounds.py relies on it."""
import ctypes as C
import os
import re

import pytest

from sparrowrecsys_amd import _lib as L
from tests.conftest import ROOT

UNSET = {1: 1, 256: 1, 257: 2, 524288: 2048, 524289: 2048}


def test_unset_the_grid_is_the_parent_commits(lib, monkeypatch):
    monkeypatch.delenv("SPRK_FE_MAX_GRID", raising=False)
    assert {n: lib.sprk_segments_grid(n) for n in UNSET} == UNSET
    assert lib.sprk_segments_grid(0) == 1 and lib.sprk_segments_grid(-5) == 1          # fe_grid: never an empty launch
    assert lib.sprk_segments_grid(2 ** 31 - 2) == 2048                                  # the most rows any entry point takes


@pytest.mark.parametrize("cap", [1, 3, 2047, 2048])
def test_set_it_caps_there(lib, monkeypatch, cap):
    monkeypatch.setenv("SPRK_FE_MAX_GRID", str(cap))
    assert {n: lib.sprk_segments_grid(n) for n in UNSET} == {n: min(g, cap) for n, g in UNSET.items()}
    assert lib.sprk_segments_grid(256 * cap) == cap and lib.sprk_segments_grid(256 * cap + 1) == cap


@pytest.mark.parametrize("value", ["0", "-1", "2049", "abc", "", "3x", "2.5", "99999999999999999999"])
def test_anything_else_is_ignored(lib, monkeypatch, value):
    monkeypatch.setenv("SPRK_FE_MAX_GRID", value)
    assert {n: lib.sprk_segments_grid(n) for n in UNSET} == UNSET


def test_it_is_read_at_each_call(lib, monkeypatch):
    monkeypatch.setenv("SPRK_FE_MAX_GRID", "3")
    assert lib.sprk_segments_grid(524289) == 3
    monkeypatch.setenv("SPRK_FE_MAX_GRID", "1")
    assert lib.sprk_segments_grid(524289) == 1
    monkeypatch.delenv("SPRK_FE_MAX_GRID")
    assert lib.sprk_segments_grid(524289) == 2048


def test_header_export_and_prototype_agree(lib):
    import subprocess
    header = open(os.path.join(ROOT, "include", "sparrow_hip.h")).read()
    assert re.search(r"\bint64_t\s+sprk_segments_grid\(int64_t items\);", header)
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "sprk_segments_grid" in {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert "sprk_segments_grid" in L.EXPORTED_SYMBOLS
    assert lib.sprk_segments_grid.argtypes == [C.c_int64] and lib.sprk_segments_grid.restype == C.c_int64


def test_no_literal_cap_is_left_beside_the_switch():
    """Every host-side cap goes through fe_max_grid(): FE_MAX_GRID is named by k_segments.h, which defines it, and host_segments.h alone."""
    csrc = os.path.join(ROOT, "sparrowrecsys_amd", "csrc")
    users = sorted(f for f in os.listdir(csrc) if "FE_MAX_GRID" in open(os.path.join(csrc, f), errors="replace").read())
    assert users == ["host_segments.h", "k_segments.h"]
