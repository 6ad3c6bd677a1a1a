// libemx, emx_summary: the kernels that reduce ONE ensemble's chain (stored, N, W) -- W = ndim, or nblobs for the blob plane --
// to its mean, ddof = 1 covariance, MAP sample and order statistics.  Included by emx_batch_summary.hip inside its anonymous
// namespace, after the helpers it shares with the batch kernels (sel_key / sel_unkey / sel_scan_bins / sel_leaders, map_better,
// tri_pair, gm_tile_samples, k_bsum_gram_fin_*).
//
// The batch kernels parallelise over members and 256-row slices; one ensemble of 65 536 walkers has neither.  Here the work is
// cut over the flat sample index i = t N + w (selected row t, walker w), n = nt N samples, and over the flat element index
// f = i W + d for the selection:
//   k_esum_mean_part   chunk c = samples [c C, c C + C): a workgroup is 256 / CW sample lanes x CW columns and walks its chunk with
//                      coalesced loads; the sample lanes are added in order -> part (G, W)
//   k_esum_fold        64 consecutive partials -> one, in order; applied until one is left.  C, G and so the whole tree are fixed
//                      by (nt, N, W): the sums have one order on every call and launch shape.  The three run twice: the
//                      second time on x - mean, which gives the residual sums r; the mean reported is mean + r / n and the
//                      covariance (G_jk - r_j r_k / n) / (n - 1), the corrected two-pass form (emx_batch_summary.hip says why)
//   k_esum_gram_small  W < 16: k_bsum_gram_small's explicit-fma form on a chunk of samples -> gpart (G, P)
//   k_esum_gram_mfma   W >= 16: k_bsum_gram_mfma's v_mfma_f64_16x16x4_f64 form on a chunk -> gpart (G, NP, 4, 64); both are
//                      folded like the mean and finished by the batch's k_bsum_gram_fin_* (one member, one slice)
//   k_esum_map_part / k_esum_map_fin   grid-wide (value, index) arg-max under map_better's total order, then the W coordinates
//   k_esum_sel_init / k_esum_hist / k_esum_scan / k_esum_compact   radix select, 8 passes of 8 bits as in the batch and the host
//                      twin.  A histogram workgroup (1024 threads) reads its share of the selection coalesced over f and counts
//                      EVERY dim it meets: its LDS holds up to 128 slots of 256 uint32 bins (a slot's bins are 257 apart, so that
//                      lanes on neighbouring dims with one digit fall on different banks), a slot being one (dim, distinct
//                      prefix) -- the ranks of a dim that still share a prefix share a slot.  Where W x (slots a dim) exceeds 128
//                      the dims go in tiles.  After pass 1 every rank's top 16 key bits are known: k_esum_compact reads the
//                      selection a third and last time and appends the elements that still match some rank of their dim to a
//                      list of (key, dim), which passes 2 ... 7 count instead.  The list's order depends on the schedule; only
//                      integer counts are taken from it.  The scan knows the list's exact length before it is written; where it
//                      would exceed a quarter of the selection (heavy ties) the remaining passes read the selection itself.
// No floating-point atomics; the integer atomics (LDS uint32, global uint64) count.
#pragma once

struct ESel {
    const double* x;      // selected row 0 of the plane (., N, W)
    const double* lp;     // selected row 0 of the log-prob plane (., N)
    int64_t N, NW, rowstep, lprowstep, n, nt;      // rowstep = stride N W, lprowstep = stride N, n = nt N samples
    int32_t W;
};

constexpr int ES_CHUNK = 1024;          // samples a chunk, times m (es_chunk)
constexpr int ES_MAX_CHUNKS = 4096;
constexpr int ES_FOLD = 64;
constexpr int ES_SLOTS = 128;           // histogram slots a workgroup (x 257 uint32)
constexpr int ES_HT = 1024;             // threads of the selection kernels
constexpr int ES_STAGE = 4 * ES_HT;     // elements a compaction round
constexpr int ES_COMPACT_TABLE = 8192;  // (dim, slot) prefixes k_esum_compact keeps in LDS
constexpr int ES_COV_MAX_W = 256;       // mu[] of the MFMA Gram kernel

// samples a chunk: a multiple of 1024 with at most gmax chunks
inline int64_t es_chunk(int64_t n, int64_t gmax) {
    const int64_t m = std::max<int64_t>(1, (n + (int64_t)ES_CHUNK * gmax - 1) / ((int64_t)ES_CHUNK * gmax));
    return m * ES_CHUNK;
}

// grid (G, column tiles of CW): part (G, W).  sub: nothing, or W values (the first mean) subtracted from every sample before it
// is added: the residual pass, in the mean's order
__global__ __launch_bounds__(256) void k_esum_mean_part(const ESel g, int64_t C, int CW, const double* __restrict__ sub, double* __restrict__ part) {
    __shared__ double red[256];
    const int tid = threadIdx.x, SPB = 256 / CW, s = tid / CW, c = tid - s * CW;
    const int64_t d = (int64_t)blockIdx.y * CW + c;
    const int64_t i0 = (int64_t)blockIdx.x * C, i1 = i0 + C < g.n ? i0 + C : g.n;
    double acc = 0.0;
    if (s < SPB && d < g.W) {
        int64_t i = i0 + s, t = i / g.N, w = i - t * g.N;
        const int64_t qstep = SPB / g.N, wstep = SPB - qstep * g.N;
        const double* p = g.x + d;
        const double m = sub ? sub[d] : 0.0;            // x - 0.0 is x
#pragma unroll 8
        for (; i < i1; i += SPB) {
            acc += p[t * g.rowstep + w * g.W] - m;
            t += qstep;
            w += wstep;
            if (w >= g.N) {
                w -= g.N;
                ++t;
            }
        }
    }
    red[tid] = acc;
    __syncthreads();
    if (s == 0 && d < g.W) {
        double tot = 0.0;
        for (int q = 0; q < SPB; ++q) tot += red[q * CW + c];
        part[(int64_t)blockIdx.x * g.W + d] = tot;
    }
}

// out[b][e] = in[64 b][e] + in[64 b + 1][e] + ... in order; grid (width / 256, groups)
__global__ __launch_bounds__(256) void k_esum_fold(const double* __restrict__ in, double* __restrict__ out, int64_t count, int64_t width) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= width) return;
    const int64_t q0 = (int64_t)blockIdx.y * ES_FOLD, q1 = q0 + ES_FOLD < count ? q0 + ES_FOLD : count;
    double acc = 0.0;
#pragma unroll 8
    for (int64_t q = q0; q < q1; ++q) acc += in[q * width + e];
    out[(int64_t)blockIdx.y * width + e] = acc;
}

// first pass (mu0 = nothing): out = sum / n, the mean the residuals and the Gram are centred on.  Residual pass: resid = sum =
// the sum of (x - mu0), out = mu0 + resid / n, the mean that is reported
__global__ __launch_bounds__(256) void k_esum_mean_fin(const double* __restrict__ sum, const double* __restrict__ mu0, double* __restrict__ out,
                                                       double* __restrict__ resid, int W, int64_t n) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= W) return;
    if (!mu0) {
        out[d] = sum[d] / (double)n;
        return;
    }
    resid[d] = sum[d];
    out[d] = isfinite(mu0[d]) ? mu0[d] + sum[d] / (double)n : mu0[d];      // a column that holds inf keeps the mean NumPy gives it
}

// W < 16.  One workgroup a chunk: gpart (G, P), P = W (W + 1) / 2
__global__ __launch_bounds__(256) void k_esum_gram_small(const ESel g, int64_t C, const double* __restrict__ mean, double* __restrict__ gpart) {
    __shared__ double tile[GS_TILE * 15];
    __shared__ double red[256];
    __shared__ double mu[16];
    const int tid = threadIdx.x, D = g.W, P = D * (D + 1) / 2, G = 256 / P;
    if (tid < D) mu[tid] = mean[tid];
    const int p = tid % P, grp = tid / P;
    int j, k;
    tri_pair(p, D, &j, &k);
    const int64_t i0 = (int64_t)blockIdx.x * C, i1 = i0 + C < g.n ? i0 + C : g.n, ns = i1 - i0;
    // this thread's next element f = i0 D + tid + 256 it as (row, col, d), advanced without a division
    const int64_t f0 = i0 * D + tid;
    int64_t row = f0 / g.NW, col = f0 - row * g.NW;
    int d = (int)(col % D);
    const int64_t qstep = 256 / g.NW, cstep = 256 - qstep * g.NW;
    const int dstep = 256 % D;
    double acc = 0.0;
    for (int64_t s0 = 0; s0 < ns; s0 += GS_TILE) {
        const int cnt = (int)(ns - s0 < GS_TILE ? ns - s0 : GS_TILE);
        const int nel = cnt * D;
        __syncthreads();                                        // the previous tile is consumed (and mu is written)
        for (int slot = tid; slot < nel; slot += 256) {
            tile[slot] = g.x[row * g.rowstep + col] - mu[d];
            row += qstep;
            col += cstep;
            if (col >= g.NW) {
                col -= g.NW;
                ++row;
            }
            d += dstep;
            if (d >= D) d -= D;
        }
        __syncthreads();
        if (grp < G)
            for (int i = grp; i < cnt; i += G) acc = fma(tile[i * D + j], tile[i * D + k], acc);
    }
    red[tid] = acc;
    __syncthreads();
    if (tid < P) {
        double tot = 0.0;
        for (int q = 0; q < G; ++q) tot += red[q * P + tid];
        gpart[(int64_t)blockIdx.x * P + tid] = tot;
    }
}

// 16 <= W <= 256.  grid (pair groups of 32, G): gpart (G, NP, 4, 64), the accumulators as k_bsum_gram_mfma leaves them
__global__ __launch_bounds__(256) void k_esum_gram_mfma(const ESel g, int64_t C, const double* __restrict__ mean, double* __restrict__ gpart, int Dp,
                                                        int NP) {
    typedef double d4 __attribute__((ext_vector_type(4)));
    __shared__ double tile[GM_TILE_DOUBLES];
    __shared__ double mu[ES_COV_MAX_W];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, D = g.W;
    const int T = gm_tile_samples(Dp), LS = Dp + 2, DPB = Dp / 16;
    for (int c = tid; c < Dp; c += 256) mu[c] = c < D ? mean[c] : 0.0;
    int ja[GM_PAIRS_WAVE], ka[GM_PAIRS_WAVE];
    bool live[GM_PAIRS_WAVE];
    d4 acc[GM_PAIRS_WAVE];
#pragma unroll
    for (int a = 0; a < GM_PAIRS_WAVE; ++a) {
        const int pi = blockIdx.x * GM_PAIRS_WG + 4 * a + wv;
        live[a] = pi < NP;
        int jb = 0, kb = 0;
        if (live[a]) tri_pair(pi, DPB, &jb, &kb);
        ja[a] = jb * 16 + (lane & 15);
        ka[a] = kb * 16 + (lane & 15);
        acc[a] = d4{0.0, 0.0, 0.0, 0.0};
    }
    const int64_t i0 = (int64_t)blockIdx.y * C, i1 = i0 + C < g.n ? i0 + C : g.n;
    // staging: a wave's lanes cover CPL columns of 64 / CPL samples at a time; T is a multiple of the 4 SPW samples the workgroup
    // stages at once, so a lane's samples are i0 + wv SPW + ls + 4 SPW it across tiles: (row, walker) advance without a division
    const int CPL = Dp <= 16 ? 16 : Dp <= 32 ? 32 : 64, SPW = 64 / CPL, step = 4 * SPW;
    const int ls = lane / CPL, c0 = lane - ls * CPL;
    int64_t si = i0 + wv * SPW + ls, row = si / g.N, w = si - row * g.N;
    const int64_t qstep = step / g.N, wstep = step - qstep * g.N;
    __syncthreads();
    for (int64_t t0 = i0; t0 < i1; t0 += T) {
        for (int i = wv * SPW + ls; i < T; i += step) {
            const bool in = si < i1;
            const double* src = g.x + row * g.rowstep + w * D;
            for (int c = c0; c < Dp; c += CPL) tile[i * LS + c] = (in && c < D) ? src[c] - mu[c] : 0.0;
            si += step;
            row += qstep;
            w += wstep;
            if (w >= g.N) {
                w -= g.N;
                ++row;
            }
        }
        __syncthreads();
        for (int ks = 0; ks < T / 4; ++ks) {
            const double* trow = tile + (ks * 4 + (lane >> 4)) * LS;
#pragma unroll
            for (int a = 0; a < GM_PAIRS_WAVE; ++a)
                if (live[a]) acc[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(trow[ja[a]], trow[ka[a]], acc[a], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < GM_PAIRS_WAVE; ++a) {
        if (!live[a]) continue;
        const int pi = blockIdx.x * GM_PAIRS_WG + 4 * a + wv;
        double* out = gpart + ((int64_t)blockIdx.y * NP + pi) * 256;
#pragma unroll
        for (int r = 0; r < 4; ++r) out[r * 64 + lane] = acc[a][r];
    }
}

// (value, index) of the best of 256 candidates, left in bv[0] / bi[0]
__device__ __forceinline__ void map_reduce_wg(double* bv, int64_t* bi, int tid) {
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h && map_better(bv[tid + h], bi[tid + h], bv[tid], bi[tid])) {
            bv[tid] = bv[tid + h];
            bi[tid] = bi[tid + h];
        }
        __syncthreads();
    }
}

// grid-stride over the flat sample index: pv / pi (gridDim.x)
__global__ __launch_bounds__(256) void k_esum_map_part(const ESel g, double* __restrict__ pv, int64_t* __restrict__ pi) {
    __shared__ double bv[256];
    __shared__ int64_t bi[256];
    const int tid = threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * 256;
    int64_t e = (int64_t)blockIdx.x * 256 + tid, row = e / g.N, w = e - row * g.N;
    const int64_t qstep = step / g.N, wstep = step - qstep * g.N;
    double best = 0.0;
    int64_t idx = -1;
#pragma unroll 4
    for (; e < g.n; e += step) {
        const double v = g.lp[row * g.lprowstep + w];
        if (idx < 0 || v > best) {
            best = v;
            idx = e;
        }
        row += qstep;
        w += wstep;
        if (w >= g.N) {
            w -= g.N;
            ++row;
        }
    }
    bv[tid] = best;
    bi[tid] = idx;
    map_reduce_wg(bv, bi, tid);
    if (tid == 0) {
        pv[blockIdx.x] = bv[0];
        pi[blockIdx.x] = bi[0];
    }
}

// one workgroup: the best of the np partials, then its W coordinates
__global__ __launch_bounds__(256) void k_esum_map_fin(const ESel g, const double* __restrict__ pv, const int64_t* __restrict__ pi, int np,
                                                      double* __restrict__ map_x, double* __restrict__ map_lp) {
    __shared__ double bv[256];
    __shared__ int64_t bi[256];
    const int tid = threadIdx.x;
    double best = 0.0;
    int64_t idx = -1;
    for (int q = tid; q < np; q += 256)
        if (map_better(pv[q], pi[q], best, idx)) {
            best = pv[q];
            idx = pi[q];
        }
    bv[tid] = best;
    bi[tid] = idx;
    map_reduce_wg(bv, bi, tid);
    const int64_t e = bi[0], r = e / g.N, w = e - r * g.N;
    if (tid == 0) map_lp[0] = bv[0];
    const double* x = g.x + r * g.rowstep + w * g.W;
    for (int d = tid; d < g.W; d += 256) map_x[d] = x[d];
}

// ---- selection.  State of dim d, rank r at [d nr + r]: prefix, rem, slotof (the slot of r's leader); of dim d, slot s at
// [d nr + s]: slotpf (the prefix the slot counts), its bins hist[(d nr + s) 256 ...]; nlead[d] slots in use.
// info[0]: the most slots any dim uses; info[1]: the elements that match some slot after the scan.
__global__ __launch_bounds__(256) void k_esum_sel_init(u64* __restrict__ prefix, int64_t* __restrict__ rem, int32_t* __restrict__ slotof,
                                                       u64* __restrict__ slotpf, int32_t* __restrict__ nlead, const int64_t* __restrict__ ranks,
                                                       int nr, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int r = (int)(i % nr);
    prefix[i] = 0;
    rem[i] = ranks[r];
    slotof[i] = 0;               // every rank starts with the empty prefix: one slot a dim
    slotpf[i] = 0;
    if (r == 0) nlead[i / nr] = 1;
}

// pass `pass` (digit = bits [shift, shift + 8), shift = 56 - 8 pass) over the selection (LIST = false: elements [0, nel) of the
// flat (sample, dim) index) or over the compacted list.  grid (workgroups of `per` elements, dim tiles of DT); ns slots a dim.
template <bool LIST>
__global__ __launch_bounds__(ES_HT) void k_esum_hist(const ESel g, const u64* __restrict__ lkey, const uint32_t* __restrict__ ldim, int64_t nel,
                                                     int64_t per, const u64* __restrict__ slotpf, const int32_t* __restrict__ nlead,
                                                     u64* __restrict__ hist, int nr, int ns, int DT, int pass) {
    extern __shared__ uint32_t es_lds[];
    const int tid = threadIdx.x, W = g.W;
    const int d0 = blockIdx.y * DT, dc = W - d0 < DT ? W - d0 : DT, nslot = dc * ns, shift = 56 - 8 * pass;
    uint32_t* h = es_lds;                                                   // nslot x 257
    u64* spf = (u64*)(es_lds + ((DT * ns * 257 + 1) & ~1));                 // nslot prefixes' high bits; 2^64 - 1: unused
    for (int i = tid; i < nslot * 257; i += ES_HT) h[i] = 0;
    for (int i = tid; i < nslot; i += ES_HT) {
        const int dl = i / ns, s = i - dl * ns;
        spf[i] = s < nlead[d0 + dl] ? (pass ? slotpf[(int64_t)(d0 + dl) * nr + s] >> (shift + 8) : 0) : ~0ull;
    }
    __syncthreads();
    const int64_t f0 = (int64_t)blockIdx.x * per, f1 = f0 + per < nel ? f0 + per : nel;
    int64_t f = f0 + tid, row = 0, col = 0;
    int d = 0;
    int64_t qstep = 0, cstep = 0;
    int dstep = 0;
    if (!LIST) {
        row = f / g.NW;
        col = f - row * g.NW;
        d = (int)(col % W);
        qstep = ES_HT / g.NW;
        cstep = ES_HT - qstep * g.NW;
        dstep = ES_HT % W;
    }
#pragma unroll 4
    for (; f < f1; f += ES_HT) {
        u64 key;
        int dl;
        if (LIST) {
            key = lkey[f];
            dl = (int)ldim[f] - d0;
        } else {
            key = sel_key((u64)__double_as_longlong(g.x[row * g.rowstep + col]));
            dl = d - d0;
            row += qstep;
            col += cstep;
            if (col >= g.NW) {
                col -= g.NW;
                ++row;
            }
            d += dstep;
            if (d >= W) d -= W;
        }
        if (dl >= 0 && dl < dc) {
            const u64 hi = pass ? key >> (shift + 8) : 0;
            const uint32_t digit = (uint32_t)(key >> shift) & 255u;
            for (int s = 0; s < ns; ++s)
                if (spf[dl * ns + s] == hi) {                               // the slots of a dim hold distinct prefixes
                    atomicAdd(&h[(dl * ns + s) * 257 + digit], 1u);
                    break;
                }
        }
    }
    __syncthreads();
    for (int i = tid; i < nslot * 256; i += ES_HT) {
        const int sl = i >> 8, dl = sl / ns, s = sl - dl * ns;
        const uint32_t v = h[sl * 257 + (i & 255)];
        if (v) atomicAdd(&hist[((int64_t)(d0 + dl) * nr + s) * 256 + (i & 255)], (u64)v);
    }
}

// one thread a dim: every rank takes its digit from its slot's bins; the ranks that still share a prefix share a slot of the
// next pass.  After the last pass order (nr, W).
__global__ __launch_bounds__(64) void k_esum_scan(u64* __restrict__ prefix, int64_t* __restrict__ rem, int32_t* __restrict__ slotof,
                                                  u64* __restrict__ slotpf, int32_t* __restrict__ nlead, const u64* __restrict__ hist,
                                                  u64* __restrict__ info, double* __restrict__ order, int nr, int W, int pass) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= W) return;
    const int shift = 56 - 8 * pass;
    u64 pfx[SEL_MAX_RANKS], cnt[SEL_MAX_RANKS];
    int32_t ld[SEL_MAX_RANKS], sl[SEL_MAX_RANKS];
    for (int r = 0; r < nr; ++r) {
        int64_t want = rem[i * nr + r];
        const u64* bins = hist + (i * nr + slotof[i * nr + r]) * 256;
        const int digit = sel_scan_bins(bins, &want);
        rem[i * nr + r] = want;
        cnt[r] = bins[digit];
        pfx[r] = prefix[i * nr + r] | ((u64)digit << shift);
        prefix[i * nr + r] = pfx[r];
    }
    sel_leaders(pfx, ld, nr);
    int nl = 0;
    u64 surv = 0;
    for (int r = 0; r < nr; ++r)
        if (ld[r] == r) {
            sl[r] = nl;
            slotpf[i * nr + nl] = pfx[r];
            surv += cnt[r];
            ++nl;
        }
    for (int r = 0; r < nr; ++r) slotof[i * nr + r] = sl[ld[r]];
    nlead[i] = nl;
    atomicMax(&info[0], (u64)nl);
    atomicAdd(&info[1], surv);
    if (pass == SEL_PASSES - 1)
        for (int r = 0; r < nr; ++r) order[(int64_t)r * W + i] = __longlong_as_double((long long)sel_unkey(pfx[r]));
}

// the elements whose top `bits` key bits equal a slot's of their dim -> (lkey, ldim)[*counter ...), at most cap of them.
// W ns <= ES_COMPACT_TABLE.  grid (workgroups of `per` elements), per a multiple of ES_STAGE.
__global__ __launch_bounds__(ES_HT) void k_esum_compact(const ESel g, int64_t nel, int64_t per, const u64* __restrict__ slotpf,
                                                        const int32_t* __restrict__ nlead, int nr, int ns, int bits, u64* __restrict__ lkey,
                                                        uint32_t* __restrict__ ldim, u64* __restrict__ counter, u64 cap) {
    extern __shared__ uint32_t es_lds[];
    __shared__ uint32_t scount;
    __shared__ u64 sbase;
    const int tid = threadIdx.x, W = g.W;
    u64* spf = (u64*)es_lds;                    // W ns
    u64* skey = spf + W * ns;                   // ES_STAGE
    uint32_t* sdim = (uint32_t*)(skey + ES_STAGE);
    for (int i = tid; i < W * ns; i += ES_HT) {
        const int dd = i / ns, s = i - dd * ns;
        spf[i] = s < nlead[dd] ? slotpf[(int64_t)dd * nr + s] >> (64 - bits) : ~0ull;
    }
    if (tid == 0) scount = 0;
    __syncthreads();
    const int64_t f0 = (int64_t)blockIdx.x * per, f1 = f0 + per < nel ? f0 + per : nel;
    int64_t f = f0 + tid, row = f / g.NW, col = f - row * g.NW;
    int d = (int)(col % W);
    const int64_t qstep = ES_HT / g.NW, cstep = ES_HT - qstep * g.NW;
    const int dstep = ES_HT % W;
    for (int64_t fb = f0; fb < f1; fb += ES_STAGE) {
#pragma unroll
        for (int k = 0; k < ES_STAGE / ES_HT; ++k) {
            if (f < f1) {
                const u64 key = sel_key((u64)__double_as_longlong(g.x[row * g.rowstep + col])), hi = key >> (64 - bits);
                bool hit = false;
                for (int s = 0; s < ns; ++s) hit = hit || spf[d * ns + s] == hi;
                if (hit) {
                    const uint32_t at = atomicAdd(&scount, 1u);
                    skey[at] = key;
                    sdim[at] = (uint32_t)d;
                }
            }
            f += ES_HT;
            row += qstep;
            col += cstep;
            if (col >= g.NW) {
                col -= g.NW;
                ++row;
            }
            d += dstep;
            if (d >= W) d -= W;
        }
        __syncthreads();
        const uint32_t cnt = scount;
        if (tid == 0 && cnt) sbase = atomicAdd(counter, (u64)cnt);
        __syncthreads();
        for (uint32_t i = tid; i < cnt; i += ES_HT) {
            const u64 at = sbase + i;
            if (at < cap) {
                lkey[at] = skey[i];
                ldim[at] = sdim[i];
            }
        }
        if (tid == 0) scount = 0;
        __syncthreads();
    }
}
