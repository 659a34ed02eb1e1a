// hashgan_amd -- tie-aware AP at the top-R cut (He, Cakir, Bargal, Sclaroff, CVPR 2018): the expectation of the reference's AP@R
// (lib/metric.py:19-23) over all orders inside the Hamming tie groups, the chance that the top R hold a hit at all, and the exact
// minimum and maximum of AP over those orders.  All of it is a function of the two columns hg_rel_hist leaves per query --
// n_d = all[d] rows at distance d, r_d = rel[d] relevant ones among them -- and R: no select, no lists, no ranking.
//
// k_tie_ap, one workgroup of 256 threads per (query, cut-off):
//   1  thread d reads n_d, r_d; block scan -> P_d (rows before group d), S_d (relevant rows before it); r_d / n_d and
//      rho_d = (r_d - 1) / (n_d - 1) once per group; the cut group t is the one with P_t < R <= P_t + n_t, c = R - P_t.
//   2  thread x walks the ranks x + 1, x + 257, ... <= R (its group index only ever moves forward) and adds, for a rank inside a
//      whole group, the rank's terms of I, I_max, I_min, and for a rank inside the cut group those of T0, T1.  The five sums are
//      reduced by a butterfly inside each wavefront and in wavefront order across the four.
//   3  the h pass, serial, one lane each of the four wavefronts side by side:
//        wave 0  hypergeometric weights from the mode upwards (ratio recurrence, w(mode) = 1) with their sums
//        wave 1  the same from mode - 1 downwards
//        wave 2  Bmax(h) as a running sum and the maximum of (I_max + Bmax(h)) / (S + h)
//        wave 3  Bmin(h) by its recurrence and the minimum of (I_min + Bmin(h)) / (S + h)
//      Thread 0 joins the two sides (upwards first) and writes the seven results.
// Every term is non-negative and is added as it stands; float64, plain divisions (correctly rounded), no fused multiply-add
// (-ffp-contract=off).  The order of every addition is a function of the two columns and R: not of Q, not of timing, no atomics.
#pragma once
#include "hg_graded.hpp"

namespace hg {

constexpr int TA_THREADS = 256;        // one thread per distance in step 1: b <= 255
constexpr int TA_MAX_R = 64;           // cut-offs per pass

struct TieApArgs {
    const u32* all; const u32* rel;    // hg_rel_hist's tables [NB][Qpad]
    const i64* Rs;                     // [nR] ascending cut-offs, 1 <= R <= N
    double* ap_exp; double* p_hit; double* ap_min; double* ap_max; double* rel_exp;   // [Q][nR]
    i64* rel_lo; i64* rel_hi;          // [Q][nR]
    i64 Qpad;
    int NB, nR;
};

// the five position sums, every lane ends with the same bits
__device__ __forceinline__ double ta_block_sum(double v, double* s4, const int lane, const int wave) {
    v = wave_sum_f64(v);
    if (lane == 0) s4[wave] = v;
    __syncthreads();
    return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

static __global__ __launch_bounds__(TA_THREADS) void k_tie_ap(const TieApArgs a) {
    __shared__ u32 sn[TA_THREADS], sr[TA_THREADS], sP[TA_THREADS], sS[TA_THREADS];
    __shared__ double sfrac[TA_THREADS], srho[TA_THREADS];
    __shared__ u32 wn[TA_THREADS / 64], wr[TA_THREADS / 64];
    __shared__ double red[5][TA_THREADS / 64];
    __shared__ double hres[8];         // the h pass: [0..2] upwards {W, W_hit, A}, [3..5] downwards, [6] max, [7] min
    __shared__ int st;
    const int q = (int)blockIdx.x, j = (int)blockIdx.y;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const i64 R = a.Rs[j];

    // 1: the columns, their exclusive scans, the cut group
    const u32 n = tid < a.NB ? a.all[(i64)tid * a.Qpad + q] : 0u;
    const u32 r = tid < a.NB ? a.rel[(i64)tid * a.Qpad + q] : 0u;
    const u32 in = wave_scan_u32(n, lane), ir = wave_scan_u32(r, lane);
    if (lane == 63) { wn[wave] = in; wr[wave] = ir; }
    if (tid == 0) st = 0;
    __syncthreads();
    u32 bn = 0, br = 0;
#pragma unroll
    for (int w = 0; w < TA_THREADS / 64; ++w) {
        bn += w < wave ? wn[w] : 0u;
        br += w < wave ? wr[w] : 0u;
    }
    const u32 Pd = bn + in - n, Sd = br + ir - r;
    sn[tid] = n; sr[tid] = r; sP[tid] = Pd; sS[tid] = Sd;
    sfrac[tid] = r > 0u ? (double)r / (double)n : 0.0;
    srho[tid] = r > 0u && n > 1u ? (double)(r - 1u) / (double)(n - 1u) : 0.0;
    if (n > 0u && (i64)Pd < R && R <= (i64)Pd + (i64)n) st = tid;      // (exactly one group: 1 <= R <= N)
    __syncthreads();
    const int t = st;
    const i64 P = sP[t], S = sS[t], nt = sn[t], rt = sr[t];
    const i64 c = R - P;

    // 2: one sweep over the ranks 1..R
    double aI = 0.0, aMax = 0.0, aMin = 0.0, aT0 = 0.0, aT1 = 0.0;
    {
        int d = 0;
        for (i64 p = tid; p < R; p += TA_THREADS) {
            while (d < t && p >= (i64)sP[d] + (i64)sn[d]) ++d;         // (p < R <= P_t + n_t: stops at t at the latest)
            const i64 i = p - (i64)sP[d] + 1;                          // place inside the group, 1..n_d
            const double k = (double)(p + 1);
            if (d < t) {
                const i64 nd = sn[d], rd = sr[d], Sg = sS[d];
                if (rd > 0) {
                    aI += sfrac[d] * (((double)(Sg + 1) + (double)(i - 1) * srho[d]) / k);
                    if (i <= rd) aMax += (double)(Sg + i) / k;
                    if (i > nd - rd) aMin += (double)(Sg + i - (nd - rd)) / k;
                }
            } else {
                aT0 += 1.0 / k;
                aT1 += (double)(i - 1) / k;
            }
        }
    }
    const double I = ta_block_sum(aI, red[0], lane, wave);
    const double Imax = ta_block_sum(aMax, red[1], lane, wave);
    const double Imin = ta_block_sum(aMin, red[2], lane, wave);
    const double T0 = ta_block_sum(aT0, red[3], lane, wave);
    const double T1 = ta_block_sum(aT1, red[4], lane, wave);

    // 3: the h pass
    const i64 nr = nt - rt;                                            // irrelevant rows of the cut group
    const i64 h_lo = c > nr ? c - nr : 0, h_hi = c < rt ? c : rt;
    if (lane == 0) {
        if (wave < 2) {
            i64 m = (i64)(((u64)(c + 1) * (u64)(rt + 1)) / (u64)(nt + 2));   // the mode of the hypergeometric
            m = m < h_lo ? h_lo : (m > h_hi ? h_hi : m);
            const double base = (double)(S + 1) * T0;
            const double cm1 = (double)(c - 1);
            double W = 0.0, Wh = 0.0, A = 0.0, w = 1.0;
            const i64 first = wave == 0 ? m : m - 1, step = wave == 0 ? 1 : -1;
            for (i64 h = first; h >= h_lo && h <= h_hi; h += step) {
                if (h != m) {
                    // w(h) / w(h - 1) = (r - h + 1)(c - h + 1) / (h (n - r - c + h)); downwards its reciprocal at h + 1
                    const u64 up = wave == 0 ? (u64)(rt - h + 1) * (u64)(c - h + 1) : (u64)(h + 1) * (u64)(nr - c + h + 1);
                    const u64 dn = wave == 0 ? (u64)h * (u64)(nr - c + h) : (u64)(rt - h) * (u64)(c - h);
                    w = w * ((double)up / (double)dn);
                    if (w == 0.0) break;                               // (underflow: every weight further out is zero too)
                }
                W += w;
                if (S + h > 0) {
                    double B = 0.0;
                    if (h > 0) {
                        const double sl = c > 1 ? (double)(h - 1) / cm1 : 0.0;
                        B = ((double)h / (double)c) * (base + sl * T1);
                    }
                    Wh += w;
                    A += w * ((I + B) / (double)(S + h));
                }
            }
            hres[wave * 3 + 0] = W; hres[wave * 3 + 1] = Wh; hres[wave * 3 + 2] = A;
        } else if (wave == 2) {
            double B = 0.0, best = __builtin_nan("");
            bool have = false;
            if (h_lo == 0 && S > 0) { best = Imax / (double)S; have = true; }
            for (i64 h = 1; h <= h_hi; ++h) {
                B += (double)(S + h) / (double)(P + h);
                if (h >= h_lo) {
                    const double v = (Imax + B) / (double)(S + h);
                    best = have && best >= v ? best : v;
                    have = true;
                }
            }
            hres[6] = best;
        } else {
            double B = 0.0, U = 0.0, best = __builtin_nan("");
            bool have = false;
            if (h_lo == 0 && S > 0) { best = Imin / (double)S; have = true; }
            if (nr == 0) {
                // a cut group of relevant rows only: h = c, first and last coincide, Bmin(c) = Bmax(c) -- by wave 2's sum, so that
                // a ranking whose tie groups are all label-pure has ap_min == ap_max to the bit
                for (i64 h = 1; h <= c; ++h) B += (double)(S + h) / (double)(P + h);
                best = (Imin + B) / (double)(S + c);
            }
            for (i64 h = 0; h < h_hi && nr > 0; ++h) {                 // Bmin(h) -> Bmin(h + 1)
                const double x = (double)(P + c - h);
                U += 1.0 / x;
                B += (double)S / x + U;
                if (h + 1 >= h_lo) {
                    const double v = (Imin + B) / (double)(S + h + 1);
                    best = have && best <= v ? best : v;
                    have = true;
                }
            }
            hres[7] = best;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const double W = hres[0] + hres[3], Wh = hres[1] + hres[4], A = hres[2] + hres[5];
        const i64 o = (i64)q * a.nR + j;
        a.p_hit[o] = Wh / W;
        a.ap_exp[o] = Wh > 0.0 ? A / Wh : __builtin_nan("");
        a.ap_max[o] = hres[6];
        a.ap_min[o] = hres[7];
        a.rel_exp[o] = (double)S + (double)((u64)c * (u64)rt) / (double)nt;
        a.rel_lo[o] = S + h_lo;
        a.rel_hi[o] = S + h_hi;
    }
}

}  // namespace hg
