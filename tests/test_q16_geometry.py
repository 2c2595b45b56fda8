"""The 16-bit dedup tables take any number of buckets: geometry and the cut of a hashed id into (bucket, entry), on the host alone.

tests/q16_check.cpp — a stand-alone program over pgvectorscale_amd/csrc/vs_q16.h, the one header the launch planning and the kernel
share — is compiled with the host compiler under the address and undefined-behaviour sanitizers and walks every x < 2^qd of every
legal (n, gcap) pair: bucket < gcap / 8, entry < 2^16, join(bucket, entry) == x, and the id hash inverts.  The expected geometry is
restated here independently of the header.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (2, 3, 1_000, 4_001, 65_536, 65_537, 4_000_000, 50_000_000)
GCAPS = (1_024, 1_280, 2_304, 4_608, 12_800, 20_736, 32_768)
# qd = 32 (more than 2^31 rows): the one width at which the magic multiplier can be inexact, so the geometry checks the error term
# and may refuse; walked by sample (every 251st x and both sides of every bucket boundary)
BIG = [(n, g) for n in (2_147_483_649, 3_000_000_000, 4_294_967_295) for g in (262_144, 524_288, 524_544, 786_432, 1_000_192, 4_194_304)]


def clog2(v):
    return max(v - 1, 0).bit_length()


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("q16") / "q16_check")
    subprocess.check_call([cxx, "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pgvectorscale_amd", "csrc"), os.path.join(ROOT, "tests", "q16_check.cpp"), "-o", exe])
    args = [str(v) for n in NS for g in GCAPS for v in (n, g)] + [str(v) for pair in BIG for v in pair]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines[0].split() == ["products", "1", "1"]  # VS_Q16_A * VS_Q16_AI == VS_Q16_B * VS_Q16_BI == 1 mod 2^32
    rows = {}
    for ln in lines[1:]:
        v = [int(t) for t in ln.split()]
        rows[(v[0], v[1])] = dict(zip(("ok", "qd", "qe", "qm", "qs", "ocap", "vwords", "gregion", "sb", "bad_bucket", "bad_entry", "bad_inverse",
                                       "bad_hash"), v[2:]))
    assert len(rows) == len(NS) * len(GCAPS) + len(BIG)
    return rows


@pytest.mark.parametrize("gcap", GCAPS)
@pytest.mark.parametrize("n", NS)
def test_geometry_and_cut(report, n, gcap):
    r = report[(n, gcap)]
    nb = gcap // 8
    qd = max(clog2(max(n, 2)), clog2(nb) + 3, 1)
    assert r["qd"] == qd
    # accepted exactly when an entry fits 16 bits: at least 2^(qd - 16) buckets
    assert bool(r["ok"]) == (nb >= 2 ** max(qd - 16, 0)), r
    # sized from the real gcap, nothing rounded up to a power of two
    ocap = max(-(-(gcap // 16) // 128) * 128, 256)
    assert (r["ocap"], r["vwords"], r["gregion"]) == (ocap, (gcap + ocap) // 32, gcap // 2 + ocap)
    assert 2 ** (r["sb"] - 1) < gcap + ocap <= 2 ** r["sb"]
    if not r["ok"]:
        return
    assert r["qe"] == -(-(2 ** qd) // nb) and 8 <= r["qe"] <= 65536
    assert 2 ** r["qs"] < r["qe"] <= 2 ** (r["qs"] + 1) and r["qm"] == -(-(2 ** (32 + r["qs"])) // r["qe"]) < 2 ** 32
    if nb & (nb - 1) == 0:  # a power-of-two bucket count goes through the same code and is the plain shift it used to be
        assert r["qm"] == 2 ** 31 and r["qe"] == 2 ** (qd - clog2(nb))
    # over all x < 2^qd
    assert (r["bad_bucket"], r["bad_entry"], r["bad_inverse"], r["bad_hash"]) == (0, 0, 0, 0), r


def test_some_pairs_are_refused(report):
    # (the pairs above cover both answers: 50M rows need at least 1 024 buckets, 4M rows at least 64)
    assert not report[(50_000_000, 4_608)]["ok"] and report[(50_000_000, 12_800)]["ok"] and report[(4_000_000, 1_024)]["ok"]


def _magic(qd, nb):
    """restated: qe, qs, qm and whether floor(x qm / 2^(32 + qs)) == floor(x / qe) is guaranteed for every x < 2^qd"""
    qe = -(-(2 ** qd) // nb)
    qs = (qe - 1).bit_length() - 1  # 2^qs < qe <= 2^(qs + 1)
    two = 2 ** (32 + qs)
    qm = -(-two // qe)
    return qe, qs, qm, qe <= 65536 and qm < 2 ** 32 and (qm * qe - two) * 2 ** qd <= two


@pytest.mark.parametrize("n,gcap", BIG)
def test_thirty_two_hashed_bits(report, n, gcap):
    r = report[(n, gcap)]
    nb = gcap // 8
    assert r["qd"] == 32
    qe, qs, qm, exact = _magic(32, nb)
    assert bool(r["ok"]) == exact, (r, qe, qs, qm)
    if nb < 2 ** 16:
        assert not r["ok"]  # an entry would need more than 16 bits
    if r["ok"]:
        assert (r["qe"], r["qs"], r["qm"]) == (qe, qs, qm)
        assert (r["bad_bucket"], r["bad_entry"], r["bad_inverse"], r["bad_hash"]) == (0, 0, 0, 0), r


def test_thirty_two_hashed_bits_cover_both_answers(report):
    big = [report[p] for p in BIG if p[1] // 8 >= 2 ** 16]
    assert any(r["ok"] for r in big) and any(not r["ok"] for r in big)  # (refused by the error term alone: enough buckets, inexact magic)
    assert report[(3_000_000_000, 524_544)]["ok"]  # ... and a bucket count that is no power of two is accepted and walked
