// libemx, emx_chain_minmax / emx_histograms: the kernels that bin ONE ensemble's chain (stored, N, W) -- W = ndim, or nblobs for
// the blob plane -- into the marginal histogram of every column and the 2-d histogram of every requested column pair, next to
// the chain.  Included by emx_batch_summary.hip inside its anonymous namespace, after emx_summary_single.hpp (ESel, u64).
//
// The bin edges come from the host (np.linspace there, or the caller's own) and are never recomputed here: a value v falls in
// bin b iff e[b] <= v < e[b + 1], the last bin closed on the right -- np.histogram's rule; NaN and everything outside fall
// nowhere.  Every accumulation is an integer add (LDS uint32, global uint64 atomics): no count depends on the launch shape, the
// chunking or the order of the atomics.
//   k_hist_minmax   per column min / max of the finite values and the number of non-finite ones over a chunk of samples; a
//                   workgroup is 256 / CW sample lanes x CW columns (coalesced over f = sample W + d, a lane keeps its column)
//                   -> partials (G, W), folded by k_hist_minmax_fin.  min / max are exact whatever the order.
//   k_hist_code     one coalesced pass over a chunk of selected rows for a TILE of columns [d0, d0 + dc): the tile's edges
//                   (marginal and pair) and its marginal counters live in LDS, as many columns as 128 KB hold; every value is
//                   binary-searched against its column's edges, counted, and its pair-bin code (uint8, 255: outside) goes
//                   through an LDS transpose into the dim-major code plane (W, Mp) so that the chain is read AND the codes are
//                   written coalesced.  The tiles partition the columns: together they read the chain once, whatever the pairs.
//   k_hist_pair     a workgroup owns one panel (i, j) for one slice of the chunk's samples: pb_i x pb_j uint32 counters in LDS
//                   (<= 64 KB), the two code rows streamed 16 bytes a lane.
#pragma once

constexpr int EH_MAX_BINS = 1024;         // marginal bins a column
constexpr int EH_MAX_PAIR_BINS = 128;     // pair bins a column: codes 0 ... 127, a panel's counters <= 64 KB
constexpr int EH_OUT = 255;               // the code of a value outside its column's pair edges
constexpr int EH_T = 1024;                // threads of k_hist_code
constexpr int EH_K = 16;                  // rounds of SPB samples between two write-outs of the staged codes
constexpr int EH_MAX_TILE_COLS = 256;     // columns a tile: at least 4 sample lanes, the staged codes <= 17 KB
constexpr size_t EH_LDS_TABLES = (size_t)128 << 10;      // edges + counters of a tile

// grid (G chunks of C samples, column tiles of CW): plo / phi / pnf (G, W)
__global__ __launch_bounds__(256) void k_hist_minmax(const ESel g, int64_t C, int CW, double* __restrict__ plo, double* __restrict__ phi,
                                                     u64* __restrict__ pnf) {
    __shared__ double rlo[256], rhi[256];
    __shared__ u64 rnf[256];
    const int tid = threadIdx.x, SPB = 256 / CW, s = tid / CW, c = tid - s * CW;
    const int64_t d = (int64_t)blockIdx.y * CW + c;
    const int64_t i0 = (int64_t)blockIdx.x * C, i1 = i0 + C < g.n ? i0 + C : g.n;
    double lo = INFINITY, hi = -INFINITY;
    u64 nf = 0;
    if (s < SPB && d < g.W) {
        int64_t i = i0 + s, t = i / g.N, w = i - t * g.N;
        const int64_t qstep = SPB / g.N, wstep = SPB - qstep * g.N;
        const double* p = g.x + d;
#pragma unroll 8
        for (; i < i1; i += SPB) {
            const double v = p[t * g.rowstep + w * g.W];
            if (v - v == 0.0) {                                 // finite
                lo = fmin(lo, v);
                hi = fmax(hi, v);
            } else {
                ++nf;
            }
            t += qstep;
            w += wstep;
            if (w >= g.N) {
                w -= g.N;
                ++t;
            }
        }
    }
    rlo[tid] = lo;
    rhi[tid] = hi;
    rnf[tid] = nf;
    __syncthreads();
    if (s == 0 && d < g.W) {
        for (int q = 1; q < SPB; ++q) {
            lo = fmin(lo, rlo[q * CW + c]);
            hi = fmax(hi, rhi[q * CW + c]);
            nf += rnf[q * CW + c];
        }
        plo[(int64_t)blockIdx.x * g.W + d] = lo;
        phi[(int64_t)blockIdx.x * g.W + d] = hi;
        pnf[(int64_t)blockIdx.x * g.W + d] = nf;
    }
}

// one thread a column: the G partials -> lo / hi / nf (W)
__global__ __launch_bounds__(256) void k_hist_minmax_fin(const double* __restrict__ plo, const double* __restrict__ phi, const u64* __restrict__ pnf,
                                                         int64_t G, int W, double* __restrict__ lo_out, double* __restrict__ hi_out,
                                                         u64* __restrict__ nf_out) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= W) return;
    double lo = INFINITY, hi = -INFINITY;
    u64 nf = 0;
    for (int64_t q = 0; q < G; ++q) {
        lo = fmin(lo, plo[q * W + d]);
        hi = fmax(hi, phi[q * W + d]);
        nf += pnf[q * W + d];
    }
    lo_out[d] = lo;
    hi_out[d] = hi;
    nf_out[d] = nf;
}

// the bin of v in the nb bins of e[0 ... nb], -1: none (NaN, outside)
__device__ __forceinline__ int eh_bin(const double* e, int nb, double v) {
    if (!(v >= e[0]) || !(v <= e[nb])) return -1;
    int lo = 0, hi = nb;                          // e[lo] <= v, and v < e[hi] or hi == nb
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (v >= e[mid])
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// One chunk of selected rows (M = rows N samples, sample i = (row i / N, walker i % N)) and one tile of columns.
struct EHCode {
    const double* x;                // the chunk's first selected row of the plane: element (t, w, d) at x[t rowstep + w W + d]
    int64_t N, rowstep, M, per;     // per: samples a workgroup, a multiple of EH_K SPB (and so of 16)
    int32_t W, d0, dc, same;        // same: the pair edges ARE the marginal edges (one search a value)
    const int64_t* edge_off;        // (W + 1) into edges; column d has edge_off[d + 1] - edge_off[d] - 1 bins
    const int64_t* pedge_off;       // the same of the pair edges
    const double* edges;
    const double* pedges;
    u64* counts;                    // column d's marginal counters at edge_off[d] - d
    uint8_t* codes;                 // (W, Mp), or nullptr: no pairs, nothing but the marginals
    int64_t Mp;                     // a multiple of 16
};

// dynamic LDS of a tile: nme marginal edges, npe pair edges of its own, nme - dc counters, the staged codes
__host__ __device__ inline size_t eh_code_lds(int64_t nme, int64_t npe, int dc, bool codes) {
    const int SPB = EH_T / dc, TSP = EH_K * SPB + 4;
    return (size_t)(nme + npe) * 8 + (size_t)((nme - dc + 3) & ~(int64_t)3) * 4 + (codes ? (size_t)dc * TSP : 0);
}

// grid (workgroups of `per` samples)
__global__ __launch_bounds__(EH_T) void k_hist_code(const EHCode g) {
    extern __shared__ __attribute__((aligned(16))) double eh_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, dc = g.dc;
    const int SPB = EH_T / dc, TS = EH_K * SPB, TSP = TS + 4;
    const bool pairs = g.codes != nullptr, own = pairs && !g.same;
    const int64_t e0 = g.edge_off[g.d0], p0 = own ? g.pedge_off[g.d0] : 0;
    const int nme = (int)(g.edge_off[g.d0 + dc] - e0), npe = own ? (int)(g.pedge_off[g.d0 + dc] - p0) : 0, ncnt = nme - dc;
    double* me = eh_lds;
    double* pe = me + nme;
    uint32_t* cnt = (uint32_t*)(pe + npe);
    uint8_t* stage = (uint8_t*)(cnt + ((ncnt + 3) & ~3));           // dc rows of TSP bytes, 4-byte aligned
    for (int i = tid; i < nme; i += EH_T) me[i] = g.edges[e0 + i];
    for (int i = tid; i < npe; i += EH_T) pe[i] = g.pedges[p0 + i];
    for (int i = tid; i < ncnt; i += EH_T) cnt[i] = 0;
    // thread (sample lane s0, column c) keeps its column: its edges and counters stay where they are for the whole chunk
    const int s0 = tid / dc, c = tid - s0 * dc;
    const bool active = s0 < SPB;
    int nb = 1, pb = 1, co = 0;
    const double* medge = me;
    const double* pedge = me;
    if (active) {
        const int d = g.d0 + c, mo = (int)(g.edge_off[d] - e0);
        nb = (int)(g.edge_off[d + 1] - g.edge_off[d]) - 1;
        medge = me + mo;
        co = mo - c;
        if (own) {
            pedge = pe + (int)(g.pedge_off[d] - p0);
            pb = (int)(g.pedge_off[d + 1] - g.pedge_off[d]) - 1;
        }
    }
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * g.per, i1 = i0 + g.per < g.M ? i0 + g.per : g.M;
    int64_t i = i0 + s0, t = i / g.N, w = i - t * g.N;
    const int64_t qstep = SPB / g.N, wstep = SPB - qstep * g.N;
    const double* px = g.x + g.d0 + c;
    for (int64_t base = i0; base < i1; base += TS) {
        double v[EH_K];
        const int64_t ifirst = i;
#pragma unroll
        for (int k = 0; k < EH_K; ++k) {
            v[k] = (active && i < i1) ? px[t * g.rowstep + w * g.W] : 0.0;
            i += SPB;
            t += qstep;
            w += wstep;
            if (w >= g.N) {
                w -= g.N;
                ++t;
            }
        }
#pragma unroll
        for (int k = 0; k < EH_K; ++k) {
            if (active && ifirst + (int64_t)k * SPB < i1) {
                const int b = eh_bin(medge, nb, v[k]);
                if (b >= 0) atomicAdd(&cnt[co + b], 1u);
                if (pairs) {
                    const int q = own ? eh_bin(pedge, pb, v[k]) : b;
                    stage[c * TSP + s0 + k * SPB] = (uint8_t)(q < 0 ? EH_OUT : q);
                }
            }
        }
        if (pairs) {
            __syncthreads();
            const int n = (int)(i1 - base < TS ? i1 - base : TS);
            // wave wv writes out the rows of columns wv, wv + 16, ...: 4 bytes a lane
            for (int cc = wv; cc < dc; cc += EH_T / 64) {
                uint8_t* dst = g.codes + (int64_t)(g.d0 + cc) * g.Mp + base;
                const uint8_t* src = stage + cc * TSP;
                for (int s = lane * 4; s < n; s += 256) {
                    if (s + 4 <= n) {
                        *(uint32_t*)(dst + s) = *(const uint32_t*)(src + s);
                    } else {
                        for (int q = s; q < n; ++q) dst[q] = src[q];
                    }
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    u64* out = g.counts + (e0 - g.d0);
    for (int j = tid; j < ncnt; j += EH_T)
        if (cnt[j]) atomicAdd(&out[j], (u64)cnt[j]);
}

struct EHPair {
    const uint8_t* codes;           // (W, Mp)
    int64_t Mp, M, per;             // per: samples a slice, a multiple of 16
    const int32_t* pairs;           // (P, 2)
    const int64_t* pair_off;        // (P + 1): panel p's counters at pair_off[p], pb_i x pb_j of them, column i the slow axis
    const int64_t* pedge_off;
    u64* out;
};

// grid (P, slices)
__global__ __launch_bounds__(256) void k_hist_pair(const EHPair g) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ehp_lds[];
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int a = g.pairs[2 * p], b = g.pairs[2 * p + 1];
    const uint32_t pba = (uint32_t)(g.pedge_off[a + 1] - g.pedge_off[a]) - 1u, pbb = (uint32_t)(g.pedge_off[b + 1] - g.pedge_off[b]) - 1u;
    const int nbin = (int)(pba * pbb);
    for (int i = tid; i < nbin; i += 256) ehp_lds[i] = 0;
    __syncthreads();
    const int64_t s0 = (int64_t)blockIdx.y * g.per, s1 = s0 + g.per < g.M ? s0 + g.per : g.M;
    const uint4* ra = (const uint4*)(g.codes + (int64_t)a * g.Mp);
    const uint4* rb = (const uint4*)(g.codes + (int64_t)b * g.Mp);
    for (int64_t q = s0 / 16 + tid; q * 16 < s1; q += 256) {
        const uint4 va = ra[q], vb = rb[q];
        const uint32_t wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
        const int lim = (int)(s1 - q * 16 < 16 ? s1 - q * 16 : 16);       // the bytes behind the chunk's last sample are not codes
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t ca = (wa[k >> 2] >> (8 * (k & 3))) & 255u, cb = (wb[k >> 2] >> (8 * (k & 3))) & 255u;
            if (k < lim && ca < pba && cb < pbb) atomicAdd(&ehp_lds[ca * pbb + cb], 1u);      // EH_OUT is no bin of either
        }
    }
    __syncthreads();
    u64* out = g.out + g.pair_off[p];
    for (int i = tid; i < nbin; i += 256)
        if (ehp_lds[i]) atomicAdd(&out[i], (u64)ehp_lds[i]);
}
