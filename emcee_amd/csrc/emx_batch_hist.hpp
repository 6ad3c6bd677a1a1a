// libemx, emx_chain_minmax_batch / emx_histograms_batch: the kernels that bin the chains of MANY members of an emx_batch -- the
// member-major plane (B, cap, N, W), W = ndim or nblobs -- into every member's marginal histograms and pair panels, next to the
// chain.  Included by emx_batch_summary.hip inside its anonymous namespace, after emx_hist.hpp (eh_bin, the EH_ constants, u64).
//
// A member's selected rows are the (rows, N, W) geometry of emx_hist.hpp: member z of a launch starts at x + z xstep, its rows lie
// rowstep doubles apart.  What is new is the member axis: ONE grid covers every member of a chunk (the member is a grid
// dimension), each member has its own edges (or all share one set: edge step 0) and its own counters, so the number of launches
// does not grow with the number of members.  The rule is emx_hist.hpp's: v falls in bin b iff e[b] <= v < e[b + 1], the last
// bin closed on the right; NaN and everything outside fall nowhere.  Every accumulation is an integer add (LDS uint32, global
// uint64 atomics): no count depends on the launch shape, the member chunking, the member range or the order of the atomics.
//   k_bhist_minmax  grid (slices, column tiles of CW, members): per (member, column) the min / max of the finite values and the
//                   number of non-finite ones over a slice of the member's samples; a workgroup is 256 / CW sample lanes x CW
//                   columns (coalesced over f = sample W + d) -> partials (members, slices, W), folded by k_bhist_minmax_fin, one
//                   thread a (member, column).  min / max are exact whatever the order, so the slices may follow the batch's size.
//   k_bhist_code    grid (slices, members) for a TILE of columns [d0, d0 + dc): the member's edges for the tile (marginal and
//                   pair) and its uint32 marginal counters live in LDS; every value is binary-searched against its column's
//                   edges, counted, and -- when pairs are asked for -- its one-byte pair-bin code (255: outside) goes through an
//                   LDS transpose into the member's dim-major code plane (members, W, Mp), so that the chain is read AND the codes
//                   are written coalesced.  The tiles partition the columns: together they read the chain once, whatever the pairs.
//                   The LDS counters are flushed with 64-bit integer atomics into the member's counters.
//   k_bhist_pair    grid (panels, slices, members): pb_i x pb_j uint32 counters in LDS (<= 64 KB), the member's two code rows
//                   streamed 16 bytes a lane.  A panel counted by ONE workgroup (one slice, one chunk of rows) is stored, not
//                   added: 8 coalesced bytes a counter instead of an atomic.
// Sizing: members are often small (32 x 5 x 5 000: 160 000 samples of 5 columns), so the host cuts a member into as many slices
// as fill the device from the members of the chunk (about 2 048 workgroups in all) and into no more: a workgroup of k_bhist_code
// runs at least two rounds of EH_K x (EH_T / dc) samples when there are that many, and with thousands of members a member is one
// slice.  LDS atomics on one counter serialise; a wave's 64 lanes hold EH_T / dc different samples of each of dc columns, so at
// most 64 / dc ... 64 lanes meet on one bin, as in k_hist_code.
#pragma once

struct BHMinMax {
    const double* x;                // member 0 of the launch, its first selected row
    int64_t xstep;                  // doubles from a member to the next: cap N W
    int64_t N, rowstep, n, per;     // n = rows N samples a member; per: samples a slice
    int32_t W, S;                   // S: slices a member
};

// grid (S, column tiles of CW, members): plo / phi / pnf (members, S, W)
__global__ __launch_bounds__(256) void k_bhist_minmax(const BHMinMax g, int CW, double* __restrict__ plo, double* __restrict__ phi,
                                                      u64* __restrict__ pnf) {
    __shared__ double rlo[256], rhi[256];
    __shared__ u64 rnf[256];
    const int tid = threadIdx.x, SPB = 256 / CW, s = tid / CW, c = tid - s * CW;
    const int64_t d = (int64_t)blockIdx.y * CW + c;
    const int64_t i0 = (int64_t)blockIdx.x * g.per, i1 = i0 + g.per < g.n ? i0 + g.per : g.n;
    double lo = INFINITY, hi = -INFINITY;
    u64 nf = 0;
    if (s < SPB && d < g.W) {
        int64_t i = i0 + s, t = i / g.N, w = i - t * g.N;
        const int64_t qstep = SPB / g.N, wstep = SPB - qstep * g.N;
        const double* p = g.x + (int64_t)blockIdx.z * g.xstep + d;
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
        const int64_t at = ((int64_t)blockIdx.z * g.S + blockIdx.x) * g.W + d;
        plo[at] = lo;
        phi[at] = hi;
        pnf[at] = nf;
    }
}

// one thread a (member, column): the S partials -> lo / hi / nf (members, W)
__global__ __launch_bounds__(256) void k_bhist_minmax_fin(const double* __restrict__ plo, const double* __restrict__ phi,
                                                          const u64* __restrict__ pnf, int64_t S, int64_t W, int64_t count,
                                                          double* __restrict__ lo_out, double* __restrict__ hi_out, u64* __restrict__ nf_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int64_t m = i / W, d = i - m * W;
    double lo = INFINITY, hi = -INFINITY;
    u64 nf = 0;
    for (int64_t q = 0; q < S; ++q) {
        const int64_t at = (m * S + q) * W + d;
        lo = fmin(lo, plo[at]);
        hi = fmax(hi, phi[at]);
        nf += pnf[at];
    }
    lo_out[i] = lo;
    hi_out[i] = hi;
    nf_out[i] = nf;
}

// One chunk of rows (M = rows N samples a member, sample i = (row i / N, walker i % N)) of the members of a launch and one tile of
// columns.  Member z = blockIdx.y reads x + z xstep, edges + z estep, pedges + z pstep; it counts into counts + z cstep and
// writes its codes at codes + z W Mp.
struct BHCode {
    const double* x;                // member 0 of the launch, the chunk's first selected row: element (t, w, d) at [t rowstep + w W + d]
    int64_t xstep;
    int64_t N, rowstep, M, per;     // per: samples a workgroup, a multiple of EH_K SPB (and so of 16)
    int32_t W, d0, dc, same;        // same: the pair edges ARE the marginal edges (one search a value)
    const int64_t* edge_off;        // (W + 1) into a member's edges, common to all members
    const int64_t* pedge_off;
    const double* edges;
    const double* pedges;
    int64_t estep, pstep;           // doubles from a member's edges to the next member's; 0: one set for all
    u64* counts;                    // a member's column d counts at edge_off[d] - d
    int64_t cstep;                  // edge_off[W] - W
    uint8_t* codes;                 // (members, W, Mp), or nullptr: no pairs, nothing but the marginals
    int64_t Mp;                     // a multiple of 16
};

// grid (workgroups of `per` samples, members); dynamic LDS eh_code_lds(...) as k_hist_code
__global__ __launch_bounds__(EH_T) void k_bhist_code(const BHCode g) {
    extern __shared__ __attribute__((aligned(16))) double bh_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, dc = g.dc;
    const int SPB = EH_T / dc, TS = EH_K * SPB, TSP = TS + 4;
    const int64_t z = blockIdx.y;
    const bool pairs = g.codes != nullptr, own = pairs && !g.same;
    const int64_t e0 = g.edge_off[g.d0], p0 = own ? g.pedge_off[g.d0] : 0;
    const int nme = (int)(g.edge_off[g.d0 + dc] - e0), npe = own ? (int)(g.pedge_off[g.d0 + dc] - p0) : 0, ncnt = nme - dc;
    double* me = bh_lds;
    double* pe = me + nme;
    uint32_t* cnt = (uint32_t*)(pe + npe);
    uint8_t* stage = (uint8_t*)(cnt + ((ncnt + 3) & ~3));           // dc rows of TSP bytes, 4-byte aligned
    const double* ge = g.edges + z * g.estep + e0;
    const double* gp = g.pedges + z * g.pstep + p0;
    for (int i = tid; i < nme; i += EH_T) me[i] = ge[i];
    for (int i = tid; i < npe; i += EH_T) pe[i] = gp[i];
    for (int i = tid; i < ncnt; i += EH_T) cnt[i] = 0;
    // thread (sample lane s0, column c) keeps its column: its edges and counters stay where they are for the whole slice
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
    const double* px = g.x + z * g.xstep + g.d0 + c;
    uint8_t* codes = pairs ? g.codes + z * g.W * g.Mp : nullptr;
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
                uint8_t* dst = codes + (int64_t)(g.d0 + cc) * g.Mp + base;
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
    u64* out = g.counts + z * g.cstep + (e0 - g.d0);
    for (int j = tid; j < ncnt; j += EH_T)
        if (cnt[j]) atomicAdd(&out[j], (u64)cnt[j]);
}

struct BHPair {
    const uint8_t* codes;           // (members, W, Mp)
    int64_t Mp, M, per;             // per: samples a slice, a multiple of 16
    int32_t W, store;               // store: a panel is counted by this workgroup alone -- its counters are stored, zeros too
    const int32_t* pairs;           // (P, 2)
    const int64_t* pair_off;        // (P + 1): panel p's counters at pair_off[p], pb_i x pb_j of them, column i the slow axis
    const int64_t* pedge_off;
    u64* out;                       // (members, pair_off[P])
    int64_t ostep;                  // pair_off[P]
};

// grid (P, slices, members)
__global__ __launch_bounds__(256) void k_bhist_pair(const BHPair g) {
    extern __shared__ __attribute__((aligned(16))) uint32_t bhp_lds[];
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.x, z = blockIdx.z;
    const int a = g.pairs[2 * p], b = g.pairs[2 * p + 1];
    const uint32_t pba = (uint32_t)(g.pedge_off[a + 1] - g.pedge_off[a]) - 1u, pbb = (uint32_t)(g.pedge_off[b + 1] - g.pedge_off[b]) - 1u;
    const int nbin = (int)(pba * pbb);
    for (int i = tid; i < nbin; i += 256) bhp_lds[i] = 0;
    __syncthreads();
    const int64_t s0 = (int64_t)blockIdx.y * g.per, s1 = s0 + g.per < g.M ? s0 + g.per : g.M;
    const uint8_t* plane = g.codes + z * g.W * g.Mp;
    const uint4* ra = (const uint4*)(plane + (int64_t)a * g.Mp);
    const uint4* rb = (const uint4*)(plane + (int64_t)b * g.Mp);
    for (int64_t q = s0 / 16 + tid; q * 16 < s1; q += 256) {
        const uint4 va = ra[q], vb = rb[q];
        const uint32_t wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
        const int lim = (int)(s1 - q * 16 < 16 ? s1 - q * 16 : 16);       // the bytes behind the chunk's last sample are not codes
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t ca = (wa[k >> 2] >> (8 * (k & 3))) & 255u, cb = (wb[k >> 2] >> (8 * (k & 3))) & 255u;
            if (k < lim && ca < pba && cb < pbb) atomicAdd(&bhp_lds[ca * pbb + cb], 1u);      // EH_OUT is no bin of either
        }
    }
    __syncthreads();
    u64* out = g.out + z * g.ostep + g.pair_off[p];
    if (g.store) {
        for (int i = tid; i < nbin; i += 256) out[i] = (u64)bhp_lds[i];
    } else {
        for (int i = tid; i < nbin; i += 256)
            if (bhp_lds[i]) atomicAdd(&out[i], (u64)bhp_lds[i]);
    }
}
