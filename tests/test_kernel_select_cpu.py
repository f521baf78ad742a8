"""The kernel-selection rule (navbot_ppo_amd/csrc/navsim_select.h) without a GPU: the header compiles alone with g++, and what it
picks -- for the eight stepping entry points, over envs x beams x maps x movers x sensor options x navsim_set_shape's overrides --
is the table beside this file, which was generated from the functions the rule replaced (pick_epb, pick_shape, pick_rollout, the
bit arithmetic of navsim_set_map and the launch ladders of the entry points, as they stood before the rule became a module)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(REPO, "navbot_ppo_amd", "csrc")


def _dump(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC] + flags +
                          [os.path.join(HERE, "kernel_select_dump.cpp"), "-o", str(exe)])
    return exe


@pytest.fixture(scope="module")
def table():
    rows = open(os.path.join(HERE, "kernel_select_table.txt")).read().splitlines()
    assert 300 <= len(rows) <= 999
    return rows


def test_header_needs_no_hip():
    """g++ sees no HIP header: the rule is plain host C++"""
    txt = open(os.path.join(CSRC, "navsim_select.h")).read()
    assert "hip" not in txt.replace("navsim.hip", "").lower().split("#pragma once")[1].split("namespace navsim_select")[0]
    assert shutil.which("g++")


def test_picks_match_the_table(tmp_path, table):
    exe = _dump(tmp_path, "dump", ["-O1"])
    got = subprocess.check_output([str(exe), "table"], text=True).splitlines()
    assert len(got) == len(table)
    for g, want in zip(got, table):
        assert g == want
    # the table holds every boundary of the rule: each value of each axis of the grid
    cols = list(zip(*(r.split(" | ")[0].split() for r in table)))
    assert set(cols[0]) == {"1", "15", "16", "17", "4095", "4096", "4097", "8192", "8193", "16383", "16384", "65536"}
    assert set(cols[1]) == {"10", "36"}
    assert {(s, p) for s, p in zip(cols[2], cols[3])} == {(str(s), "0") for s in (8, 32, 33, 64, 65, 2048, 4096, 4097)} | {
        (str(s), "1") for s in (64, 128, 1536)}
    assert set(cols[4]) == set(cols[5]) == set(cols[7]) == {"0", "1"}
    assert set(cols[6]) == {"0", "4", "8", "16", "32", "64"}
    # ... and the full grid is the table's rows and 18 more between each two
    full = subprocess.check_output([str(exe), "full"], text=True).splitlines()
    assert full[::19] == table and len(full) == 8640


def test_picks_under_sanitizers(tmp_path, table):
    """the same program under AddressSanitizer and UBSan (a plain executable: nothing is preloaded)"""
    exe = _dump(tmp_path, "dump_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([str(exe), "full"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    assert r.stdout.splitlines()[::19] == table
