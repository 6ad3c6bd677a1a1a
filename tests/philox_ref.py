"""Reference of the native (Philox mode) stream's decision-bearing draws, NumPy only: nothing here comes from emcee_amd, and no
value is fitted to what the library gives.  Philox4x32 itself is gauss_noise_ref.philox4x32, an independent restatement checked
on its own (tests/test_gauss_noise_ref_cpu.py).

THE CONTRACT (`EMX_RNG_PHILOX`; csrc/emx_rng.hpp, native_slot / native_gauss_slot / native_move_choice in
csrc/emx_kernels.hpp, csrc/emx_pt.hpp, emx_host_walk_kde_draws in csrc/emx.hip)

Every draw is some of the four 32-bit words of ONE Philox4x32-10 block under the key (seed lo, seed hi) of the chain's 64-bit
seed.  There are two counter layouts:

* walker-keyed  (walker, stream, step lo, step hi)   -- what a walker draws for itself at a step;
* step-keyed    (step lo, step hi, tag, index)       -- what a step draws for the whole ensemble; the tags are the ASCII words
  'PERM' 0x5045524d, 'SWPM' 0x5357504d, 'SWAP' 0x53574150, 'MOVE' 0x4d4f5645, 'FACT' 0x46414354.

Two numbers are made from words:

* u53(a, b) = ((a >> 5) 2^26 + (b >> 6)) 2^-53 in [0, 1): 27 high bits of a, 26 high bits of b, exact in float64;
* bounded64(a, b, n) = floor(r n / 2^64) with r = a 2^32 + b: a uniform integer of [0, n) (bias below n 2^-64).  For n < 2^32
  this is ((a n + ((b n) >> 32)) >> 32), the form the library evaluates: r n = a n 2^32 + b n, so
  floor(r n / 2^64) = floor((a n + b n / 2^32) / 2^32) = floor((a n + floor(b n / 2^32)) / 2^32), because for an integer x and
  a real y >= 0, floor((x + y) / m) = floor((x + floor(y)) / m) (the fraction of y cannot carry x + floor(y) over a multiple of
  m); nothing overflows 64 bits: a n + (2^32 - 1) <= (2^32 - 1)^2 + 2^32 - 1 < 2^64.  bounded64_wide() is the 128-bit product
  in Python integers; the CPU tests hold the two forms to each other.

THE SPLIT.  The S sub-ensembles have the sizes of `arange(N) % S`: set s has floor(N / S) + (s < N mod S) members.  The split
of step `step` is a keyed bijection pi of [0, N): walker w belongs to set pi(w) mod S and is member number floor(pi(w) / S) of
it.  The key has a tag and an index c: with A = block(step lo, step hi, tag, c) and B = block(step lo, step hi, tag, c + 1),

    m1, c1, m2, c2 = A[0], A[1], A[2], A[3];  m3, c3 = B[0], B[1];  each multiplier's low three bits forced to 101 (5 mod 8);
    bits = the smallest k >= 1 with 2^k >= N,  mask = 2^bits - 1,  s1 = ceil(bits / 2),  s2 = ceil(bits / 3);
    mix(x) = three rounds  x <- (m x + c) mod 2^bits,  x <- x xor (x >> s)  with (m, c, s) = (m1, c1, s1), (m2, c2, s2), (m3, c3, s1);
    pi(w) = the first of mix(w), mix(mix(w)), ... below N (cycle walking);  pi^-1 likewise with the inverse of mix.

The split permutation is tag 'PERM', index 0.  (It is a bijection from a small keyed family with exact set sizes -- NOT a uniform
shuffle: profiles/philox_split_statistics.md.)

A PLAN lists, split after split and member number after member number, the walker (order), up to three partners (p0, p1, p2), a
scalar (s0) and the accept uniform (uacc); off[s] is the first position of set s.  Of the walker's streams 0, 1, 2:

* uacc = u53 of words 2-3 of stream 0, for every move;
* a complement RANK r of a walker of set s counts the members of the other sets in ascending set order, member numbers ascending
  within a set; Nc = N - (size of s);
* stretch:  u = u53 of words 0-1 of stream 0;  s0 = ((a - 1) u + 1)^2 / a, each operation one IEEE float64 operation (the library
  multiplies by 1 / a when a is a power of two: the same bits);  p0 = the walker at rank bounded64(words 0-1 of stream 1, Nc);
* DE:  r1 = bounded64(words 0-1 of stream 1, Nc), r2 = bounded64(words 2-3 of stream 1, Nc - 1), r2 += 1 where r2 >= r1;  p0, p1 the
  walkers at ranks r1, r2;  u1 = 1 - u53(words 0-1 of stream 2) in (0, 1], u2 = u53(words 2-3 of stream 2);
  g = sqrt(-2 ln u1) cos(2 pi u2);  s0 = g0 (1 + sigma g).  (Needs Nc >= 2.)
* snooker (S >= 4):  the first three other sets in ascending order, j_0 < j_1 < j_2; member q is member number
  bounded64(word pair q, size of j_q) of set j_q, the word pairs being words 0-1 of stream 1, words 2-3 of stream 1, words 0-1 of
  stream 2;  the role index is floor(6 w / 2^32) of word w = word 2 of stream 2, and (p0, p1, p2) is the members permuted by the
  role-th permutation of (0, 1, 2) in lexicographic order;
* EVAL (WalkMove, KDEMove): order and uacc only; the partners are the walker itself, s0 = 0.  Their other draws:
  KDE centre = the walker at rank bounded64(words 0-1 of stream 0, Nc);  Floyd's sample of s distinct ranks: draw k = 0 ... s - 1 is
  c = bounded64(words (2h, 2h + 1) of stream 0x48000000 + (k >> 1), Nc - s + k + 1), h = k & 1, and takes rank Nc - s + k if c was
  taken before, else c;  normal pair p = (rad cos(ang), rad sin(ang)) from stream 0x4E000000 + p as DE's g is made (u1 from words
  0-1, u2 from words 2-3); a walk with s helpers takes s normals per walker, the whole-complement walk and the KDE move ndim.
* Gaussian move: every walker is its own position (order = arange(N), one set); uacc as above; in `random` mode the coordinate
  that moves is p0 = bounded64(words 0-1 of stream 0, ndim).  (Streams 2 ... of the Gaussian move are its noise: gauss_noise_ref.)

STEP-KEYED DRAWS.  'MOVE', index 0: u = u53(words 0-1); the step's move is the first k with u < cdf[k] (the last move if none).
'FACT', index 0: u = u53(words 0-1); the Gaussian move's step-size factor is exp(-l + 2 l u), l = ln(factor).
Tempering, swap pair i = 1 ... T - 1 (rung i against rung i - 1) after step `step`, under the group's rung-0 seed: the pairing is
the bijection pi_i of [0, N) with tag 'SWPM', index 2 (i - 1) (so that its two blocks, indices 2 (i - 1) and 2 (i - 1) + 1, are
its own), walker k of rung i meets walker pi_i(k) of rung i - 1; its uniform is u53(words 0-1) of ('SWAP', (i - 1) N + k).

THE TRANSCENDENTALS.  g and the normals go through the platform's log, sqrt, cos and sin; here they are evaluated in np.longdouble
(64-bit significand) from the exact u1, u2.  The library's value differs from the true one by at most, in units of 2^-52 rad
(rad = sqrt(-2 ln u1)):

    the angle: the library forms fl(fl(2 pi) u2); |fl(2 pi) - 2 pi| = 2.45e-16 and the product's rounding is at most half an ulp
        of a number below 8, 2^-51: together below 2 pi 2^-53, which moves cos / sin by at most that        pi     = 3.15
    log:  one ulp of ln u1 is a relative 2^-52 of it at most; the square root halves a relative error                0.5
    sqrt: one ulp of rad (the product -2 ln u1 is exact)                                                             1
    cos / sin: one unit allowed, i.e. two ulp of a number below 1                                                   1
    the product rad cos: one ulp of |g| <= rad                                                                       1
                                                                                                              sum:  6.65 <= 8

hence |g - g_ref| <= 8 2^-52 rad (G_BOUND_UNITS).  Through s0 = g0 (1 + sigma g): the rounding of sigma g is 2^-53 |sigma| rad at
most (0.5 more of the units: 7.15 <= 8), of 1 + sigma g and of the last product together 2^-52 |s0| at most, so
|s0 - s0_ref| <= |g0 sigma| 8 2^-52 rad + 2^-52 |s0_ref|.

THE WORD AUDIT.  Every draw goes through block(), which reports to an Audit the (counter, word) pairs it consumes.  Within one
layout distinct (walker, stream) or (tag, index) are distinct counters; the five tags differ, and 'SWAP's index (i - 1) N + k stays
below 2^32 (no wrap, hence no repeat) for T <= 256 rungs and N <= 2^24.  The two layouts can meet in one way only: a walker-keyed
counter (w, stream, lo, hi) equals a step-keyed (lo', hi', tag, index) when lo = tag, i.e. AT A STEP WHOSE LOW WORD EQUALS A TAG
(and whose high word is the index), for the walker w = lo' and stream = hi' of a step (lo', hi').  With lo' = lo that is walker
number `tag` > 1.29e9 of an ensemble, at a step beyond 1.29e9: theoretical.
"""
import contextlib

import numpy as np

from gauss_noise_ref import philox4x32

TAG_PERM, TAG_SWPM, TAG_SWAP, TAG_MOVE, TAG_FACT = (int.from_bytes(t, "big") for t in (b"PERM", b"SWPM", b"SWAP", b"MOVE", b"FACT"))
STEP_TAGS = dict(PERM=TAG_PERM, SWPM=TAG_SWPM, SWAP=TAG_SWAP, MOVE=TAG_MOVE, FACT=TAG_FACT)
STREAM_HELPER, STREAM_NORMAL = 0x48000000, 0x4E000000
ROUNDS = 10
G_BOUND_UNITS = 8.0

U64 = np.uint64
M32 = U64(0xFFFFFFFF)

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs a long double wider than float64"
TWO_PI_LD = LD(8) * np.arctan(LD(1))

# ---- mutants: one plausible mistake each, switched on by `with mutant(kind):` (tests/test_philox_ref_cpu.py) --------------------
MUTANTS = ("mul_swapped", "weyl_swapped", "rounds9", "counter_step_walker", "uacc_words01", "u53_shifts", "bounded_one_word",
           "r2_gt", "bits_n_plus_1", "mult_unforced", "s2_is_s1", "snooker_table", "partner_own_set", "swap_index_i",
           "swpm_c3")
_mutant = None


@contextlib.contextmanager
def mutant(kind):
    global _mutant
    assert kind in MUTANTS, kind
    _mutant = kind
    try:
        yield
    finally:
        _mutant = None


def _m(kind):
    return _mutant == kind


def _philox_with(c0, c1, c2, c3, k0, k1, rounds, M0, M1, W0, W1):
    """Philox4x32 with the constants as arguments: only the mutants of the constants come here"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(c).astype(U64) & M32 for c in (c0, c1, c2, c3, k0, k1)])
    for _ in range(rounds):
        a, b = U64(M0) * c0, U64(M1) * c2
        c0, c1, c2, c3 = (b >> U64(32)) ^ c1 ^ k0, b & M32, (a >> U64(32)) ^ c3 ^ k1, a & M32
        k0, k1 = (k0 + U64(W0)) & M32, (k1 + U64(W1)) & M32
    return c0, c1, c2, c3


# ---- words ----------------------------------------------------------------------------------------------------------------------
def lohi(x):
    """a 64-bit value (Python integer or array) -> its (low, high) words as uint64"""
    x = np.asarray(x & (2 ** 64 - 1) if isinstance(x, int) else x, dtype=U64)
    return x & M32, x >> U64(32)


class Audit:
    """the (counter, word) pairs consumed, by purpose"""

    def __init__(self):
        self.rows, self.what = [], []

    def add(self, what, counter, word):
        c = np.broadcast_arrays(*[np.asarray(x, dtype=U64) for x in counter])
        r = np.stack([x.ravel() for x in c] + [np.full(c[0].size, word, dtype=U64)], axis=1)
        self.rows.append(r)
        self.what += [what] * len(r)

    def table(self):
        """-> (n, 5) uint64: c0, c1, c2, c3, word"""
        return np.concatenate(self.rows) if self.rows else np.zeros((0, 5), dtype=U64)

    def duplicates(self):
        t = self.table()
        return len(t) - len(np.unique(t, axis=0))


def block(seed, counter, use, what, audit=None):
    """the four words (uint64 arrays below 2^32) of the block at `counter` under `seed`; `use`: the words the caller consumes"""
    k0, k1 = lohi(seed)
    if _m("mul_swapped"):
        v = _philox_with(*counter, k0, k1, ROUNDS, 0xCD9E8D57, 0xD2511F53, 0x9E3779B9, 0xBB67AE85)
    elif _m("weyl_swapped"):
        v = _philox_with(*counter, k0, k1, ROUNDS, 0xD2511F53, 0xCD9E8D57, 0xBB67AE85, 0x9E3779B9)
    else:
        v = philox4x32(*counter, k0, k1, 9 if _m("rounds9") else ROUNDS)
    if audit is not None:
        for w in use:
            audit.add(what, counter, w)
    return tuple(np.asarray(x).astype(U64) for x in v)


def walker_block(seed, step, walker, stream, use, what, audit=None):
    sl, sh = lohi(step)
    counter = (sl, sh, walker, stream) if _m("counter_step_walker") else (walker, stream, sl, sh)
    return block(seed, counter, use, what, audit)


def step_block(seed, step, tag, index, use, what, audit=None):
    sl, sh = lohi(step)
    return block(seed, (sl, sh, tag, np.asarray(index, dtype=U64) & M32), use, what, audit)


def u53(a, b):
    a, b = np.asarray(a, dtype=U64), np.asarray(b, dtype=U64)
    if _m("u53_shifts"):
        return (((a >> U64(6)) << U64(27)) | (b >> U64(5))).astype(np.float64) * 2.0 ** -53
    return (((a >> U64(5)) << U64(26)) | (b >> U64(6))).astype(np.float64) * 2.0 ** -53


def bounded64(a, b, n):
    """floor((a 2^32 + b) n / 2^64) for n < 2^32 (arrays broadcast) in uint64 arithmetic: the short form of the docstring"""
    a, b, n = (np.asarray(x, dtype=U64) for x in (a, b, n))
    assert np.all(n < U64(2 ** 32))
    if _m("bounded_one_word"):          # floor(u n) with u = a 2^-32: the second word forgotten
        return ((a * n) >> U64(32)).astype(np.int64)
    return ((a * n + ((b * n) >> U64(32))) >> U64(32)).astype(np.int64)


def bounded64_wide(a, b, n):
    """the definition, in Python integers (scalars)"""
    return (((int(a) << 32) | int(b)) * int(n)) >> 64


def split_sizes(N, S):
    return np.array([N // S + (1 if s < N % S else 0) for s in range(S)], dtype=np.int64)


# ---- the keyed bijection ----------------------------------------------------------------------------------------------------------
class PermKey:
    pass


def perm_key(n, seed, step, tag=TAG_PERM, index=0, audit=None):
    """the key of the bijection of [0, n); `step` may be an array (the multipliers and offsets then have its shape)"""
    k = PermKey()
    k.n = int(n)
    span = k.n + 1 if _m("bits_n_plus_1") else k.n
    k.bits = max(1, (span - 1).bit_length())
    k.mask = U64((1 << k.bits) - 1)
    A = step_block(seed, step, tag, index, (0, 1, 2, 3), "key", audit)
    B = step_block(seed, step, tag, index + 1, (0, 1), "key", audit)
    force = (lambda m: m | U64(1)) if _m("mult_unforced") else (lambda m: (m & ~U64(7)) | U64(5))
    k.m = [force(A[0]) & k.mask, force(A[2]) & k.mask, force(B[0]) & k.mask]      # only the low `bits` bits of m and c matter
    k.c = [A[1] & k.mask, A[3] & k.mask, B[1] & k.mask]
    s1, s2 = -(-k.bits // 2), -(-k.bits // 3)
    k.s = [s1, s1 if _m("s2_is_s1") else s2, s1]
    return k


def _at(v, sel):
    """key field v (scalar-shaped or broadcast against the walkers) at the boolean selection"""
    return v if np.ndim(v) == 0 else np.broadcast_to(v, sel.shape)[sel]


def _mix(x, k, sel=None):
    for m, c, s in zip(k.m, k.c, k.s):
        if sel is not None:
            m, c = _at(m, sel), _at(c, sel)
        x = (x * m + c) & k.mask
        x = x ^ (x >> U64(s))
    return x


def _inv_mod(m, bits):
    """inverse of the odd m modulo 2^bits (arrays, bits <= 31): x <- x (2 - m x), which doubles the number of right low bits; m
    itself is right to three (m m = 1 mod 8)"""
    mod = U64((1 << bits) - 1)
    x = m & mod
    for _ in range(5):
        x = (x * ((U64(2) + mod + U64(1) - ((m * x) & mod)) & mod)) & mod
    return x


def _unmix(x, k, sel=None):
    for m, c, s in zip(k.m[::-1], k.c[::-1], k.s[::-1]):
        if sel is not None:
            m, c = _at(m, sel), _at(c, sel)
        y, sh = x, s
        while sh < k.bits:                      # undo x ^= x >> s
            x = x ^ (y >> U64(sh))
            sh += s
        x = ((x + (k.mask + U64(1)) - c) * _inv_mod(m, k.bits)) & k.mask
    return x


def _walk(x, k, f):
    x = np.asarray(x, dtype=U64)
    shape = np.broadcast(x, k.m[0]).shape
    x = np.broadcast_to(x, shape).copy()
    x = f(x, k)
    while True:
        bad = x >= U64(k.n)
        if not bad.any():
            return x.astype(np.int64)
        x[bad] = f(x[bad], k, bad)


def perm_fwd(w, k):
    return _walk(w, k, _mix)


def perm_inv(p, k):
    return _walk(p, k, _unmix)


def labels(seed, steps, walkers, N, S):
    """(len(steps), len(walkers)) set of each of `walkers` at each of `steps` (vectorised over both)"""
    k = perm_key(N, seed, np.asarray(steps, dtype=U64)[:, None])
    return perm_fwd(np.asarray(walkers, dtype=U64)[None, :], k) % S


# ---- plans ----------------------------------------------------------------------------------------------------------------------
SNOOKER_ROLES = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))          # lexicographic
_SNOOKER_ROLES_HEAP = ((0, 1, 2), (1, 0, 2), (2, 0, 1), (0, 2, 1), (1, 2, 0), (2, 1, 0))     # the mutant's order


def move(kind, S=2, a=2.0, sigma=1e-5, g0=0.3):
    return dict(kind=kind, S=S, a=a, sigma=sigma, g0=g0)


def box_muller(u1, u2):
    """-> (rad cos, rad sin, rad) in long double from the exact float64 u1 in (0, 1], u2 in [0, 1)"""
    rad = np.sqrt(LD(-2) * np.log(u1.astype(LD)))
    ang = TWO_PI_LD * u2.astype(LD)
    return rad * np.cos(ang), rad * np.sin(ang), rad


def de_ranks(B, Nc):
    """two distinct complement ranks from the words B of stream 1: the second is drawn among the Nc - 1 others"""
    r1, r2 = bounded64(B[0], B[1], Nc), bounded64(B[2], B[3], np.asarray(Nc) - 1)
    return r1, r2 + ((r2 > r1) if _m("r2_gt") else (r2 >= r1))


def plan(seed, step, N, mv, audit=None):
    """the plan of `step`: dict(off, order, p0, p1, p2, s0, uacc), the layout of emx_testlib.philox_plan.  DE adds s0_ref (long
    double) and s0_bound (the docstring's bound); stretch adds u."""
    kind, S = mv["kind"], mv["S"]
    assert 2 <= S <= N and kind in ("stretch", "de", "snooker", "eval")
    sizes = split_sizes(N, S)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    key = perm_key(N, seed, step, TAG_PERM, 0, audit)
    walker_of = perm_inv(np.arange(N), key)                      # code t S + s -> the walker that is member t of set s
    sets = [walker_of[s::S] for s in range(S)]
    assert [len(x) for x in sets] == sizes.tolist()
    order = np.concatenate(sets)
    own = np.repeat(np.arange(S), sizes)
    A = walker_block(seed, step, order, 0, (2, 3) if kind == "eval" else (0, 1, 2, 3), "A", audit)
    out = dict(off=off, order=order.astype(np.int32), s0=np.zeros(N))
    out["uacc"] = u53(A[0], A[1]) if _m("uacc_words01") else u53(A[2], A[3])
    p = [order.copy() for _ in range(3)]
    if kind != "eval":
        Nc = (N - sizes)[own]
        if _m("partner_own_set"):
            comp = [order for s in range(S)]
        else:
            comp = [np.concatenate([sets[j] for j in range(S) if j != s]) for s in range(S)]

        def at_rank(r):
            w = np.empty(N, dtype=np.int64)
            for s in range(S):
                sl = slice(off[s], off[s + 1])
                w[sl] = comp[s][r[sl]]
            return w
    if kind == "stretch":
        B = walker_block(seed, step, order, 1, (0, 1), "B", audit)
        u = u53(A[0], A[1])
        t = (mv["a"] - 1.0) * u + 1.0
        out["s0"] = t * t / mv["a"]
        out["u"] = u
        out["ranks"] = bounded64(B[0], B[1], Nc)
        p[0] = at_rank(out["ranks"])
    elif kind == "de":
        assert Nc.min() >= 2, "DE needs two distinct partners in every complement"
        B = walker_block(seed, step, order, 1, (0, 1, 2, 3), "B", audit)
        Cw = walker_block(seed, step, order, 2, (0, 1, 2, 3), "C", audit)
        r1, r2 = de_ranks(B, Nc)
        out["ranks"] = np.stack([r1, r2], axis=1)
        p[0], p[1] = at_rank(r1), at_rank(r2)
        g, _, rad = box_muller(1.0 - u53(Cw[0], Cw[1]), u53(Cw[2], Cw[3]))
        g0, sg = LD(mv["g0"]), LD(mv["sigma"])
        out["s0_ref"] = g0 * (LD(1) + sg * g)
        out["s0"] = out["s0_ref"].astype(np.float64)
        out["s0_bound"] = (np.abs(g0 * sg) * LD(G_BOUND_UNITS * 2.0 ** -52) * rad + LD(2.0 ** -52) * np.abs(out["s0_ref"])).astype(np.float64)
        out["g"], out["rad"] = g, rad
    elif kind == "snooker":
        assert S >= 4
        B = walker_block(seed, step, order, 1, (0, 1, 2, 3), "B", audit)
        Cw = walker_block(seed, step, order, 2, (0, 1, 2), "C", audit)
        pairs = ((B[0], B[1]), (B[2], B[3]), (Cw[0], Cw[1]))
        mem, mrank = np.empty((N, 3), dtype=np.int64), np.empty((N, 3), dtype=np.int64)
        for s in range(S):
            sl = slice(off[s], off[s + 1])
            for q, j in enumerate([j for j in range(S) if j != s][:3]):
                mrank[sl, q] = bounded64(pairs[q][0][sl], pairs[q][1][sl], sizes[j])
                mem[sl, q] = sets[j][mrank[sl, q]]
        role = ((Cw[2] * U64(6)) >> U64(32)).astype(np.int64)
        table = np.array(_SNOOKER_ROLES_HEAP if _m("snooker_table") else SNOOKER_ROLES)
        for q in range(3):
            p[q] = mem[np.arange(N), table[role, q]]
        out["role"], out["members"], out["ranks"] = role, mem, mrank
    out["p0"], out["p1"], out["p2"] = (x.astype(np.int32) for x in p)
    return out


def gauss_plan(seed, step, N, D, mode="random", seqcol=0, audit=None):
    """the Gaussian move's plan: every walker its own position; p0 the coordinate that moves (-1: all)"""
    w = np.arange(N)
    A = walker_block(seed, step, w, 0, (0, 1, 2, 3) if mode == "random" else (2, 3), "A", audit)
    col = bounded64(A[0], A[1], D) if mode == "random" else np.full(N, seqcol if mode == "sequential" else -1)
    i32 = w.astype(np.int32)
    return dict(off=np.array([0, N], dtype=np.int32), order=i32, p0=col.astype(np.int32), p1=i32.copy(), p2=i32.copy(),
                s0=np.zeros(N), uacc=u53(A[0], A[1]) if _m("uacc_words01") else u53(A[2], A[3]))


def factor_uniform(seed, step, audit=None):
    v = step_block(seed, step, TAG_FACT, 0, (0, 1), "FACT", audit)
    return float(u53(v[0], v[1]))


def factor(seed, step, log_factor, audit=None):
    """the Gaussian move's step-size factor of `step`: exp(-l + 2 l u)"""
    return float(np.exp(-log_factor + 2.0 * log_factor * factor_uniform(seed, step, audit)))


def move_uniform(seed, step, audit=None):
    v = step_block(seed, step, TAG_MOVE, 0, (0, 1), "MOVE", audit)
    return u53(v[0], v[1])


def move_choice(seed, step, cdf, audit=None):
    """the move of `step` (steps: an array of them): the first k with u < cdf[k], the last move if there is none"""
    u = np.asarray(move_uniform(seed, step, audit))
    reached = u[..., None] >= np.asarray(cdf, dtype=np.float64)[:-1]          # cdf[k] <= u for k = 0 ... : a leading run
    k = np.logical_and.accumulate(reached, axis=-1).sum(axis=-1)
    return int(k) if k.ndim == 0 else k


def swap_draws(seed, step, N, T, audit=None):
    """-> (perm, u), both (T - 1, N): row i - 1 holds pair i's pairing pi_i(k) and uniforms"""
    perm = np.zeros((max(T - 1, 0), N), dtype=np.int32)
    u = np.zeros((max(T - 1, 0), N))
    k = np.arange(N)
    for i in range(1, T):
        key = perm_key(N, seed, step, TAG_SWPM, (i - 1) if _m("swpm_c3") else 2 * (i - 1), audit)
        perm[i - 1] = perm_fwd(k, key)
        v = step_block(seed, step, TAG_SWAP, (i if _m("swap_index_i") else i - 1) * N + k, (0, 1), "SWAP", audit)
        u[i - 1] = u53(v[0], v[1])
    return perm, u


def walk_kde_draws(seed, step, N, D, S, split, kind, s=0, audit=None):
    """the draws of every member of `split` (plan order): -> dict(helpers (ns, nh) walkers, ranks (ns, nh), normals (ns, nz) long
    double, rad (ns, nz)).  kind 'kde': nh = 1 (the centre), nz = D;  'walk' with s >= 2 helpers: nh = nz = s;  'walk' with s = 0
    (the whole complement): nh = 0, nz = D."""
    assert kind in ("walk", "kde") and (kind == "walk" or s == 0) and s != 1
    sizes = split_sizes(N, S)
    key = perm_key(N, seed, step, TAG_PERM, 0, audit)
    walker_of = perm_inv(np.arange(N), key)
    sets = [walker_of[j::S] for j in range(S)]
    me = sets[split]
    ns, Nc = len(me), N - len(sets[split])
    comp = np.concatenate([sets[j] for j in range(S) if j != split or _m("partner_own_set")])
    nz = s if s >= 2 else D
    normals, rad = np.zeros((ns, nz + 1), dtype=LD), np.zeros((ns, nz + 1), dtype=LD)
    for pr in range((nz + 1) // 2):
        v = walker_block(seed, step, me, STREAM_NORMAL + pr, (0, 1, 2, 3), "normal", audit)
        normals[:, 2 * pr], normals[:, 2 * pr + 1], r = box_muller(1.0 - u53(v[0], v[1]), u53(v[2], v[3]))
        rad[:, 2 * pr] = rad[:, 2 * pr + 1] = r
    out = dict(normals=normals[:, :nz], rad=rad[:, :nz])
    if kind == "kde":
        v = walker_block(seed, step, me, 0, (0, 1), "centre", audit)
        ranks = bounded64(v[0], v[1], Nc)[:, None]
    elif s >= 2:
        assert s <= Nc
        ranks = np.zeros((ns, s), dtype=np.int64)
        draws = np.zeros((ns, s), dtype=np.int64)
        for k in range(s):
            h = k & 1
            v = walker_block(seed, step, me, STREAM_HELPER + (k >> 1), (2 * h, 2 * h + 1), "helper", audit)
            c = bounded64(v[2 * h], v[2 * h + 1], Nc - s + k + 1)
            taken = (ranks[:, :k] == c[:, None]).any(axis=1)
            ranks[:, k] = np.where(taken, Nc - s + k, c)
            draws[:, k] = c
        out["floyd_draws"] = draws
    else:
        ranks = np.zeros((ns, 0), dtype=np.int64)
    out["ranks"] = ranks
    out["helpers"] = comp[ranks].astype(np.int32)
    return out


def philox_seed_of(seed):
    """gauss_noise_ref.philox_seed_of: the Philox seed of a chain seeded with the integer `seed`"""
    from gauss_noise_ref import philox_seed_of as f
    return f(seed)
