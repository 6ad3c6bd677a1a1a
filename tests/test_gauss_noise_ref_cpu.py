"""tests/gauss_noise_ref.py -- the reference the device's Gaussian-move noise is held against (tests/test_gpu_gauss_noise_reference.py)
-- is itself right, and its gate can tell a wrong kernel from a right one:

* Philox4x32: the published Random123 known answers at 10 rounds, the 7-round ones of the same implementation, and the project's
  own source (csrc/emx_rng.hpp, compiled for the host by tools/ubench/philox_words.cpp) on those and on 10 000 random counters;
* the edges of the two f32 inputs;
* the distribution of the reference's normals, and their independence across pairs, blocks, walkers and steps;
* a float64 twin of the noise for each plausible kernel mistake: every one is rejected by the gate on at least 99 % of the rows;
* the rule the GPU tests rest on: on the flat target every proposal is accepted."""
import os
import subprocess

import numpy as np
import pytest

import gauss_noise_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "emcee_amd", "csrc")

# counter, key, 10 rounds (Random123's known-answer vectors), 7 rounds
KAT = [
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8), (0x5f6fb709, 0x0d893f64, 0x4f121f81, 0x4f730a48)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd), (0x5207ddc2, 0x45165e59, 0x4d8ee751, 0x8c52f662)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1), (0x4dfccaba, 0x190a87f0, 0xc47362ba, 0xb6b5242a)),
]
SEED, STEP = 0x9e3779b97f4a7c15, (5 << 32) | 77          # both halves of both are non-zero and distinct


@pytest.mark.parametrize("ctr,key,r10,r7", KAT)
def test_philox_known_answers(ctr, key, r10, r7):
    assert tuple(int(v) for v in gr.philox4x32(*ctr, *key, 10)) == r10
    assert tuple(int(v) for v in gr.philox4x32(*ctr, *key, 7)) == r7


def test_the_projects_own_philox_source_agrees(tmp_path):
    """csrc/emx_rng.hpp through g++ (built as tests/test_plan_log.py builds its tools)"""
    exe = str(tmp_path / "philox_words")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-I", CSRC,
                    os.path.join(ROOT, "tools", "ubench", "philox_words.cpp"), "-o", exe], check=True)
    rs = np.random.RandomState(7)
    rows = np.concatenate([np.array([list(ctr) + list(key) for ctr, key, _, _ in KAT], dtype=np.uint64),
                           rs.randint(0, 2 ** 32, size=(10000, 6), dtype=np.uint64)])
    text = "".join("%x %x %x %x %x %x\n" % tuple(int(v) for v in r) for r in rows)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    got = np.array([int(x, 16) for x in out], dtype=np.uint32).reshape(len(rows), 8)
    for i, (_, _, r10, r7) in enumerate(KAT):
        assert tuple(int(v) for v in got[i, :4]) == r7 and tuple(int(v) for v in got[i, 4:]) == r10
    for j, rounds in ((0, 7), (4, 10)):
        ref = np.stack(gr.philox4x32(*(rows[:, i] for i in range(6)), rounds), axis=1)
        assert np.array_equal(got[:, j:j + 4], ref), "philox4x32<%d>" % rounds


# ---- the f32 inputs ------------------------------------------------------------------------------------------------------------
def test_edges_of_the_f32_inputs():
    u, rev = gr.f32_inputs(np.array([0, 1, 2 ** 32 - 129, 2 ** 32 - 128, 2 ** 32 - 1], dtype=np.uint32),
                           np.array([0, 255, 256, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32))
    assert u[0] == np.float32(2.0 ** -33) and u[1] == np.float32(1.5 * 2.0 ** -32)
    assert u[2] < 1 and u[3] == 1 and u[4] == 1                  # a >= 2^32 - 128 rounds to 2^32 in f32
    assert rev[0] == 0 and rev[1] == 0 and rev[2] == np.float32(2.0 ** -24) and rev[3] == 0.5 and rev[4] == np.float32(1 - 2.0 ** -24)
    n0, n1, r = gr.words_to_normals(np.array([0, 2 ** 32 - 128, 2 ** 32 - 1], dtype=np.uint32), np.zeros(3, dtype=np.uint32))
    assert abs(r[0] - np.sqrt(2 * 33 * np.log(2.0))) < 1e-14 and abs(r[0] - 6.7637) < 1e-4
    assert r[1] == 0 and r[2] == 0 and n0[1] == 0 and n1[2] == 0
    assert n0[0] == r[0] and n1[0] == 0


def test_inputs_stay_in_range_and_normals_finite():
    rs = np.random.RandomState(11)
    a = np.concatenate([[0, 0, 0xffffffff, 0xffffffff], rs.randint(0, 2 ** 32, 10 ** 6, dtype=np.uint64)]).astype(np.uint32)
    b = np.concatenate([[0, 0xffffffff, 0, 0xffffffff], rs.randint(0, 2 ** 32, 10 ** 6, dtype=np.uint64)]).astype(np.uint32)
    u, rev = gr.f32_inputs(a, b)
    assert u.min() > 0 and u.max() <= 1 and rev.min() >= 0 and rev.max() < 1
    n0, n1, r = gr.words_to_normals(a, b)
    assert np.all(np.isfinite(n0)) and np.all(np.isfinite(n1)) and np.all(r >= 0) and r.max() <= 6.7638
    assert np.allclose(n0 ** 2 + n1 ** 2, r ** 2, rtol=1e-14, atol=0)


# ---- distribution --------------------------------------------------------------------------------------------------------------
def _corr(x, y):
    return float(np.corrcoef(x.ravel(), y.ravel())[0, 1])


def test_reference_normals_are_standard_normal():
    from scipy.special import ndtr
    m = 4 * 10 ** 6
    rs = np.random.RandomState(2024)
    a, b = (rs.randint(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    n0, n1, _ = gr.words_to_normals(a, b)
    z = np.sort(np.concatenate([n0, n1]))
    n = z.size
    cdf = ndtr(z)
    ks = max(np.max(np.arange(1, n + 1) / n - cdf), np.max(cdf - np.arange(n) / n))
    print("gauss-noise-reference: KS distance %.3g against %.3g at n = %d" % (ks, 1.36 / np.sqrt(n), n))
    assert ks < 1.36 / np.sqrt(n)
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2.0 / n)
    assert abs(_corr(n0, n1)) < 5 / np.sqrt(m)


def test_reference_noise_is_uncorrelated_across_halves_blocks_walkers_and_steps():
    N, D = 4096, 64
    n, _ = gr.noise(SEED, STEP, N, D)
    nxt, _ = gr.noise(SEED, STEP + 1, N, D)
    hi, _ = gr.noise(SEED, STEP + (1 << 32), N, D)
    other, _ = gr.noise(SEED + 1, STEP, N, D)
    m = N * D
    lim = 5 / np.sqrt(m / 4)                 # the smallest sample below: one coordinate of every block
    q = n.reshape(N, D // 4, 4)              # a block: coordinates 4j .. 4j + 3 = pairs 2j, 2j + 1
    for i in range(4):
        for j in range(i + 1, 4):
            assert abs(_corr(q[:, :, i], q[:, :, j])) < lim, (i, j)
    assert abs(_corr(q[:, :-1], q[:, 1:])) < lim              # consecutive blocks of a walker
    assert abs(_corr(n[:-1], n[1:])) < lim                    # consecutive walkers
    for y in (nxt, hi, other):                                # consecutive steps, the step's high word, the seed
        assert abs(_corr(n, y)) < lim
    assert abs(n.mean()) < 5 / np.sqrt(m) and abs(n.var() - 1) < 5 * np.sqrt(2.0 / m)


def test_noise_layout():
    """pair p -> coordinates 2p, 2p + 1; an odd ndim drops the last sine; rows do not depend on N or D"""
    n34, r34 = gr.noise(SEED, STEP, 8, 34)
    n7, r7 = gr.noise(SEED, STEP, 5, 7)
    assert np.array_equal(n34[:5, :7], n7) and np.array_equal(r34[:5, :7], r7)
    a, b = gr.pair_words(SEED, STEP, np.array([3]), np.array([5]))
    v = gr.philox4x32(3, 2 + 2, STEP & 0xffffffff, STEP >> 32, SEED & 0xffffffff, SEED >> 32, 7)
    assert a[0] == v[2] and b[0] == v[3]
    n0, n1, r = gr.words_to_normals(a, b)
    assert n34[3, 10] == n0[0] and n34[3, 11] == n1[0] and r34[3, 10] == r[0] == r34[3, 11]
    d, _ = gr.displacement(SEED, STEP, 8, 34, 0.25, f=1.5, col=np.arange(8))
    assert np.count_nonzero(d) == 8 and d[2, 2] == (1.5 * 0.25) * n34[2, 2]


# ---- mutants -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", gr.MUTANTS)
@pytest.mark.parametrize("N,D,G", [(32, 34, 8), (32, 7, 8)])
def test_gate_rejects_every_mutant(kind, N, D, G):
    scale = 2.0 ** -(np.arange(D) % 9)                     # distinct neighbours: an off-by-one scale index shows
    ref, r = gr.displacement(SEED, STEP, N, D, scale)
    assert np.all(gr.ratio(ref, ref, r, scale) == 0)
    bad = gr.mutant_noise(kind, SEED, STEP, N, D, G=G, scale=scale)
    rows = np.any(gr.ratio(bad, ref, r, scale) > gr.K_GATE, axis=1)
    print("gauss-noise-reference: mutant %-13s %dx%d rejected on %d of %d rows" % (kind, N, D, rows.sum(), N))
    assert rows.mean() >= 0.99


def test_gate_accepts_an_honest_f32_box_muller():
    """the same mapping evaluated wholly in float32 (NumPy's libm) passes the gate with room: the gate is not tight for a correct kernel"""
    N, D = 64, 34
    ref, r = gr.displacement(SEED, STEP, N, D, 1.0)
    w, p = np.meshgrid(np.arange(N), np.arange(D // 2), indexing="ij")
    u, rev = gr.f32_inputs(*gr.pair_words(SEED, STEP, w, p))
    rad = np.sqrt(np.float32(-2.0) * np.log(u))
    ang = np.float32(2 * np.pi) * rev
    got = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=2).reshape(N, D).astype(np.float64)
    assert rad.dtype == np.float32
    assert gr.ratio(got, ref, r, 1.0).max() < 64


# ---- the flat target -----------------------------------------------------------------------------------------------------------
def test_every_proposal_is_accepted_on_the_flat_target():
    """log-prob -0.5 * 2^-200 |x|^2, 40 steps from 0 with scales <= 1: |lp_new - lp_old| stays below 2^-150, and the accept rule
    log u < lp_new - lp_old holds for every 53-bit u < 1, whose logarithm is at most log(1 - 2^-53) < -2^-54"""
    N, D = 32, 34
    x = np.zeros((N, D))
    worst = 0.0
    for t in range(40):
        d, _ = gr.displacement(SEED, STEP + t, N, D, 1.0)
        new = x + d
        dlp = -0.5 * 2.0 ** -200 * (np.sum(new * new, axis=1) - np.sum(x * x, axis=1))
        worst = max(worst, float(np.abs(dlp).max()))
        x = new
    assert worst < 2.0 ** -150
    assert np.log(1.0 - 2.0 ** -53) < -2.0 ** -54 < -worst
    with np.errstate(divide="ignore"):
        assert np.log(0.0) < -worst
