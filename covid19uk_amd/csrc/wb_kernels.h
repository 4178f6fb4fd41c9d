// Within-/between-location infection pressure of the kept draws, formed where the burst buffer lies (include/seir_hip.h,
// "Within/between pressure shares on the device").  THE definition:
//
//   For every draw of trace slots [first, first + count), every day t of the window [T - D, T) and every location m:
//     I_t[m]   I at the start of day t: init[m][2] + sum_{u<t} (k_ei[u] - k_ir[u]), scanned as integers from the slot's
//              recorded events;  psi = theta[0] of the slot;  W_t = the context's W[t].
//     x        = I_t * invN                                         (one rounding per location)
//     F_k      = fma chain over the source rows j = k mod 4, ascending, of Cstar[j][m] * x_j, the diagonal's factor
//                replaced by 0 (k = 0 .. 3), from +0
//     self     = Cstar[m][m] * x_m
//     wi       = fma(psi W_t, self, I_t[m])                         within pressure
//     be       = psi W_t * ((F0 + F1) + (F2 + F3))                  between pressure
//     tot      = fma(psi W_t, (F0 + F1) + (F2 + F3), wi);   within = wi / tot;   between = be / tot
//   -- operation for operation what k_within_between (rt_kernels.h) computes for (psi, I_t, W_t): day t = T - 1 is the
//   reference's product (the last state, and W clipped to its last index), the other days are its generalisation.
//   k_within_between's text stays as it is (its machine code must not move); wb_x / wb_row / wb_cell below restate it, with
//   the two contractions the compiler makes there under the default contract mode written as the fma they are -- wi, and
//   tot, where `wi + be` takes be's product unrounded -- and tests/test_wb_gpu.py holds the two to the same bits.
//   A draw is DEFINED for a cell iff both fractions are finite (I = 0 everywhere gives 0 / 0).  An undefined draw is counted
//   in count[b] and folded into nothing.  Per cell, sequential in draw order, every operation rounded separately (wb_fold):
//     n        defined draws;   the reference values ref_w, ref_b are the first defined draw's (the cell's n == 0)
//     sum_w    sum (within - ref_w);  sumsq_w  sum (within - ref_w)^2;  sum_b  sum (between - ref_b)
//     gt       draws with within > between
//   National pressures per draw and day: Wn = sum_m wi, Bn = sum_m be over all cells of the day, defined or not: a 64-lane
//   butterfly per column block (wb_wave_sum, a fixed order), then the column blocks in ascending order.
//
//   k_wb_prepare<EV16>   a wave per (row, draw): sums k_ei - k_ir over [0, T - D) by a wave reduction and scans the D window
//       days by wave_incl_scan, into the plane I [ND][D][Mp] (int32, day-major: a day's x vector is contiguous; the padded
//       rows stay zero).  Loads as summary_load does, for both trace widths.
//   k_wb_trace<DT>       a workgroup owns, for one chain, 64 destination columns (lane = m) x DT window days.  The loop over
//       the batch's draws is INSIDE: a thread's cells keep their accumulators in registers across it.  Per draw the
//       workgroup puts x of its days into LDS, wave p walks the source rows j = p mod 4 ascending (one Cstar element loaded
//       once per wave and reused over the tile's days), the partials meet in LDS.  No floating-point atomics.
//   k_wb_finish          Wn, Bn [slot][b][t] = the column blocks' partials in ascending order; advances count[b].
// The day tile is 4: 72 KiB of LDS at Mp = 2048 (two workgroups to a CU), 24 KiB at UK-380; at D = 14 and 8 chains that is
// 192 workgroups.  The host bounds the I plane by the staging bound of the reproduction number (RT_STAGING_BYTES /
// SEIR_OPT_RT_STAGING_KIB), cutting a call into batches of slots.  Ordinary launches on the context stream: no hand-off
// inside a launch, no persistence, and the sampler's live workspace is not touched.
#pragma once

#include "rt_trace_kernels.h"

namespace seir {

constexpr int WB_DT = 4;                         // window days per workgroup of k_wb_trace
constexpr int WB_PREP_ROWS = 8;                  // waves (rows) per workgroup of k_wb_prepare

struct WbBufs {
    int D;                         // window days
    int t0;                        // first day of the window, T - D
    int ncb;                       // column blocks, ceil(M / 64)
    int *I;                        // [ND][D][Mp] I_t of the batch's draws over the window, zero beyond M
    double *part;                  // [ND][D][ncb][2] partial national sums of the batch (within, between)
    double *Wn, *Bn;               // [cap][B][D] national pressures per kept draw, indexed by trace slot
    double *sum_w, *sumsq_w, *ref_w, *ref_b, *sum_b;   // [B][D][M]
    uint64_t *count;               // [B] draws folded since the last reset
    uint32_t *n, *gt;              // [B][D][M] defined draws; draws with within > between
};

// grid (ceil(M / WB_PREP_ROWS), ND), 64 WB_PREP_ROWS threads; nd = slot_in_batch * B + chain
template <int EV16>
__global__ __launch_bounds__(64 * WB_PREP_ROWS) void k_wb_prepare(Dims d, Consts c, WbBufs wb,
                                                                  const void *__restrict__ tr_events, int B, int first) {
    debug_skew(d);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nd = blockIdx.y, i = blockIdx.x * WB_PREP_ROWS + wv;
    const int M = d.M, T = d.T, D = wb.D;
    if (i >= M) return;
    const int jj = nd / B, b = nd - jj * B, slot = first + jj;
    const size_t row = (((size_t)slot * B + b) * M + i) * T;
    int pre = 0;
    for (int t = lane; t < wb.t0; t += 64) {
        int k[3];
        summary_load<EV16>(tr_events, row + t, true, k);
        pre += k[1] - k[2];
    }
    for (int o = 32; o > 0; o >>= 1) pre += __shfl_xor(pre, o, 64);
    int run = (int)c.init[(size_t)i * 4 + 2] + pre;  // I at the start of day T - D
    int *out = wb.I + (size_t)nd * D * d.Mp + i;
    for (int w0 = 0; w0 < D; w0 += 64) {
        const int tw = w0 + lane;
        const bool live = tw < D;
        int k[3];
        summary_load<EV16>(tr_events, row + wb.t0 + (live ? tw : 0), live, k);
        const int v = k[1] - k[2];
        const int inc = wave_incl_scan(v, lane);
        if (live) out[(size_t)tw * d.Mp] = run + (inc - v);
        run += __builtin_amdgcn_readlane(inc, 63);
    }
}

// The cell arithmetic, with k_within_between's operations repeated one for one (rt_kernels.h:117-143):
//   wb_x     x = I / N as the product with invN
//   wb_row   one source row's term into its chain, the diagonal's factor replaced by 0
//   wb_cell  self, wi (the fma the compiler contracts `I + pw * self` to), be, tot (the fma it contracts `wi + be` to: be's
//            product enters the sum unrounded) and the two divisions
__device__ __forceinline__ double wb_x(double I, double invN) { return I * invN; }
__device__ __forceinline__ double wb_row(double F, double cjm, bool diag, double xj) { return fma(diag ? 0.0 : cjm, xj, F); }
__device__ __forceinline__ void wb_cell(double I, double pw, double cmm, double xm, double F0, double F1, double F2, double F3,
                                        double &wi, double &be, double &fw, double &fb) {
#pragma clang fp contract(off)
    const double self = cmm * xm;
    wi = fma(pw, self, I);
    const double F = (F0 + F1) + (F2 + F3);
    be = pw * F;
    const double tot = fma(pw, F, wi);
    fw = wi / tot;
    fb = be / tot;
}
__device__ __forceinline__ bool wb_finite(double v) { return fabs(v) < __builtin_inf(); }

// One defined draw into a cell's accumulators: separately rounded operations, no FMA, so that the host restates them bit for bit.
__device__ __forceinline__ void wb_fold(double fw, double fb, uint32_t &n, double &ref_w, double &sum_w, double &sumsq_w,
                                        double &ref_b, double &sum_b, uint32_t &gt) {
#pragma clang fp contract(off)
    if (n == 0u) { ref_w = fw; ref_b = fb; }
    const double dw = fw - ref_w;
    const double d2 = dw * dw;
    const double db = fb - ref_b;
    sum_w = sum_w + dw;
    sumsq_w = sumsq_w + d2;
    sum_b = sum_b + db;
    gt += fw > fb ? 1u : 0u;
    n += 1u;
}
// sum over the wave of v, by a butterfly (as rt_wave_sum): every lane ends with the same value, formed in one fixed order
__device__ __forceinline__ double wb_wave_sum(double v) {
#pragma clang fp contract(off)
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_xor(v, o, 64);
        v = v + u;
    }
    return v;
}

template <int DT>
constexpr size_t k_wb_trace_lds_bytes(int Mp) { return sizeof(double) * ((size_t)DT * Mp + 4 * DT * WAVE); }
// k_wb_trace has no static LDS: the dynamic part is all of it
static_assert(k_wb_trace_lds_bytes<WB_DT>(2048) <= 160 * 1024, "k_wb_trace's day tile must fit a workgroup's LDS at Mp = 2048");

// The one statement of the within/between contraction of a batch; k_wb_trace and k_wb_trace_cells (group_curve_kernels.h)
// are __global__ wrappers with nothing else in them.  CELLS: wi and be of every live cell also go into the planes
// Wc, Bc [count * B][D][ld], ld >= M.  Dims, Consts and WbBufs by value, as rt_trace_body takes its own.
template <int DT, bool CELLS>
__device__ __forceinline__ void wb_trace_body(Dims d, Consts c, WbBufs wb, const double *__restrict__ tr_theta, int B, int first,
                                              int count, double *__restrict__ Wc, double *__restrict__ Bc, long long ld) {
    static_assert(DT % 4 == 0 && (DT & (DT - 1)) == 0, "a wave owns the days tt = wave mod 4 of the tile");
    debug_skew(d);
    extern __shared__ double lds[];                      // x [DT][Mp] | red [4][DT][64]
    constexpr int NC = DT / 4;                           // cells per thread: days tt = cc * 4 + wave, column m
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.z, m = blockIdx.x * WAVE + lane, w0 = blockIdx.y * DT;
    const int M = d.M, D = wb.D, Mp = d.Mp;
    double *X = lds, *red = lds + (size_t)DT * Mp;
    const bool min_ = m < M;
    const int mm = min_ ? m : 0;
    const double cmm = min_ ? c.Cstar[(size_t)m * d.Kp0 + m] : 0.0;
    uint32_t n[NC], gt[NC];
    double ref_w[NC], sum_w[NC], sumsq_w[NC], ref_b[NC], sum_b[NC];
    bool live[NC];
    size_t cell[NC];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) {
        const int tw = w0 + cc * 4 + wave;
        live[cc] = min_ && tw < D;
        cell[cc] = ((size_t)b * D + (tw < D ? tw : 0)) * M + mm;
        n[cc] = gt[cc] = 0u;
        ref_w[cc] = sum_w[cc] = sumsq_w[cc] = ref_b[cc] = sum_b[cc] = 0.0;
        if (live[cc]) {
            n[cc] = wb.n[cell[cc]]; gt[cc] = wb.gt[cell[cc]];
            ref_w[cc] = wb.ref_w[cell[cc]]; sum_w[cc] = wb.sum_w[cell[cc]]; sumsq_w[cc] = wb.sumsq_w[cell[cc]];
            ref_b[cc] = wb.ref_b[cell[cc]]; sum_b[cc] = wb.sum_b[cell[cc]];
        }
    }
    for (int jd = 0; jd < count; ++jd) {
        const int nd = jd * B + b;
        const double psi = tr_theta[((size_t)(first + jd) * B + b) * d.P];
        const int *Ip = wb.I + (size_t)nd * D * Mp;
        for (int idx = threadIdx.x; idx < DT * Mp; idx += 256) {
            const int tt = idx / Mp, i = idx - tt * Mp, tw = w0 + tt;
            double x = 0.0;
            if (i < M && tw < D) x = wb_x((double)Ip[(size_t)tw * Mp + i], c.invN[i]);
            X[idx] = x;
        }
        __syncthreads();
        double F[DT];
#pragma unroll
        for (int tt = 0; tt < DT; ++tt) F[tt] = 0.0;
        for (int j = wave; j < M; j += 4) {
            const double cjm = min_ ? c.Cstar[(size_t)j * d.Kp0 + m] : 0.0;
            const bool diag = j == m;
#pragma unroll
            for (int tt = 0; tt < DT; ++tt) F[tt] = wb_row(F[tt], cjm, diag, X[tt * Mp + j]);
        }
#pragma unroll
        for (int tt = 0; tt < DT; ++tt) red[(wave * DT + tt) * WAVE + lane] = F[tt];
        // x of the cell's own row is read here, in front of the barrier: behind it another wave may already write the next draw's
        double xm[NC], Iv[NC], pw[NC];
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            const int tt = cc * 4 + wave, tw = w0 + tt;
            xm[cc] = X[tt * Mp + mm];
            Iv[cc] = live[cc] ? (double)Ip[(size_t)tw * Mp + m] : 0.0;
            pw[cc] = tw < D ? psi * c.W[wb.t0 + tw] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            const int tt = cc * 4 + wave, tw = w0 + tt;
            double wi, be, fw, fb;
            wb_cell(Iv[cc], pw[cc], cmm, xm[cc], red[(0 * DT + tt) * WAVE + lane], red[(1 * DT + tt) * WAVE + lane],
                    red[(2 * DT + tt) * WAVE + lane], red[(3 * DT + tt) * WAVE + lane], wi, be, fw, fb);
            if (live[cc] && wb_finite(fw) && wb_finite(fb))
                wb_fold(fw, fb, n[cc], ref_w[cc], sum_w[cc], sumsq_w[cc], ref_b[cc], sum_b[cc], gt[cc]);
            if constexpr (CELLS)
                if (live[cc]) {                                              // defined or not, as the national sums
                    const size_t at = ((size_t)nd * D + tw) * (size_t)ld + m;
                    Wc[at] = wi; Bc[at] = be;
                }
            const double nw = wb_wave_sum(live[cc] ? wi : 0.0), nb = wb_wave_sum(live[cc] ? be : 0.0);
            if (lane == 0 && tw < D) {
                double *p = wb.part + (((size_t)nd * D + tw) * wb.ncb + blockIdx.x) * 2;
                p[0] = nw; p[1] = nb;
            }
        }
        // the next draw's x is written behind the barrier above, its partials behind the one that follows them: red is read
        // here before this wave reaches that barrier
    }
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
        if (live[cc]) {
            wb.n[cell[cc]] = n[cc]; wb.gt[cell[cc]] = gt[cc];
            wb.ref_w[cell[cc]] = ref_w[cc]; wb.sum_w[cell[cc]] = sum_w[cc]; wb.sumsq_w[cell[cc]] = sumsq_w[cc];
            wb.ref_b[cell[cc]] = ref_b[cc]; wb.sum_b[cell[cc]] = sum_b[cc];
        }
}

// grid (ncb, ceil(D / DT), B), 256 threads.  Slots [first, first + count) of the trace; nd = 0 .. of the batch's planes.
template <int DT>
__global__ __launch_bounds__(256) void k_wb_trace(Dims d, Consts c, WbBufs wb, const double *__restrict__ tr_theta, int B,
                                                  int first, int count) {
    wb_trace_body<DT, false>(d, c, wb, tr_theta, B, first, count, nullptr, nullptr, 0);
}

// grid (ceil(count * B * D / 256)), 256 threads: the national pressures of the batch's draws from their column-block
// partials, summed in ascending block order; count[b] += count.
__global__ __launch_bounds__(256) void k_wb_finish(WbBufs wb, int B, int first, int count) {
#pragma clang fp contract(off)
    const int D = wb.D;
    const size_t n = (size_t)count * B * D, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < n) {
        const double *p = wb.part + idx * wb.ncb * 2;    // idx = (nd * D + tw), nd = jd * B + b: the slot-major order of Wn, Bn
        double vw = p[0], vb = p[1];
        for (int cb = 1; cb < wb.ncb; ++cb) { vw = vw + p[2 * cb]; vb = vb + p[2 * cb + 1]; }
        wb.Wn[(size_t)first * B * D + idx] = vw;
        wb.Bn[(size_t)first * B * D + idx] = vb;
    }
    if (blockIdx.x == 0)
        for (int b = threadIdx.x; b < B; b += 256) wb.count[b] += (uint64_t)count;
}

}  // namespace seir
