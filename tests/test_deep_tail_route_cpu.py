"""CPU: how conv3d_deep.hip shares the pairs of its last, partly filled round (deep_tail in values_amd/csrc/conv3d_route.h) -- a
table of (P pairs, G workgroups) -> (full rounds, rest, split, first pair of the rest), computed by a stand-alone host program
under ASan / UBSan (nothing loaded into this process)."""
import os
import subprocess

import pytest

from tests.helpers import build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def expected(P, G, cap=4):
    """the rule as the design states it: F = P // G whole rounds, r = P - F G pairs left; S = the largest of {4, 2} with r S <= G
    (and S <= cap), else 1; r = 0 gives S = 1"""
    F = P // G
    r = P - F * G
    S = 1
    if r:
        for s in (4, 2):
            if s <= cap and r * s <= G:
                S = s
                break
    return F, r, S, F * G


def rows(G):
    return [640, 320, 128, 2560, 1, G - 1, G, G + 1, G + G // 2 + 1]


# the table, spelled out for the two grids (256 and 304 workgroups): (P, G) -> (F, r, S, tail0)
TABLE = {
    (640, 256): (2, 128, 2, 512), (320, 256): (1, 64, 4, 256), (128, 256): (0, 128, 2, 0), (2560, 256): (10, 0, 1, 2560),
    (1, 256): (0, 1, 4, 0), (255, 256): (0, 255, 1, 0), (256, 256): (1, 0, 1, 256), (257, 256): (1, 1, 4, 256),
    (385, 256): (1, 129, 1, 256),
    (640, 304): (2, 32, 4, 608), (320, 304): (1, 16, 4, 304), (128, 304): (0, 128, 2, 0), (2560, 304): (8, 128, 2, 2432),
    (1, 304): (0, 1, 4, 0), (303, 304): (0, 303, 1, 0), (304, 304): (1, 0, 1, 304), (305, 304): (1, 1, 4, 304),
    (457, 304): (1, 153, 1, 304),
}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("deep_tail") / "deep_tail_host")
    build_host_program(os.path.join(ROOT, "tests", "deep_tail_host.cpp"), exe)
    return exe


def run(host, triples):
    res = subprocess.run([host], input="".join("%d %d %d\n" % t for t in triples), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr + res.stdout
    out = res.stdout.splitlines()
    got = {}
    for ln in out[:-1]:
        P, G, cap, full, rest, split, tail0, grid = map(int, ln.split())
        got[(P, G, cap)] = (full, rest, split, tail0, grid)
    return got, out[-1]


def test_table_has_the_rows_of_both_grids():
    assert sorted(TABLE) == sorted((P, G) for G in (256, 304) for P in rows(G))
    for (P, G), want in TABLE.items():
        assert want == expected(P, G), (P, G)


def test_deep_tail_table_under_asan_ubsan(host):
    got, walked = run(host, [(P, G, 4) for P, G in TABLE])
    for (P, G), (F, r, S, tail0) in TABLE.items():
        full, rest, split, t0, grid = got[(P, G, 4)]
        assert (full, rest, split, t0) == (F, r, S, tail0), (P, G)
        assert grid == (G if F else r * S), (P, G)         # no whole round: only the workgroups that have a part are launched
    w = walked.split()
    assert w[0] == "walked" and int(w[1]) > 10 ** 4 and w[2] == "unsound" and int(w[3]) == 0, walked


def test_statistics_launches_split_no_further_than_their_entries(host):
    """a statistics launch shares a pair among at most as many workgroups as its tile's block of the partials buffer holds entries
    (cap = deep_stat_parts(stat_epc)): cap 2 turns every S = 4 row into S = 2, cap 1 leaves the launch as it was"""
    got, _ = run(host, [(P, G, cap) for P, G in TABLE for cap in (1, 2)])
    for (P, G) in TABLE:
        for cap in (1, 2):
            F, r, S, tail0 = expected(P, G, cap)
            assert S <= cap
            assert got[(P, G, cap)][:4] == (F, r, S, tail0), (P, G, cap)
