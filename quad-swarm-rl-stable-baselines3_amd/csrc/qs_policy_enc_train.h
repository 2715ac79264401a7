// qs_policy_enc_train.h -- the PPO update's MLP-family encoders (QuadMultiEncoder with the mlp, mean_embed or no
// neighbour encoder) on the split-f16 matrix cores: what qs_policy_enc.h is to the rollout, for PPOTrainer.train.  Per
// tower, from the minibatch's raw observations to the feed_forward output [B, 2H]:
//   forward   enc_mlp_train_x3_kernel: enc_mlp_x3_kernel's phase sequence and arithmetic (64 agents per block, branches in
//             the order self, neighbour, obstacle, the feed_forward accumulated part by part, the deep-sets mean a
//             register sum), written out a second time for the reason qs_policy_tail_train.h gives (a shared body would
//             carry the save sink's address arithmetic into the rollout instance).  It differs in one thing: every tanh
//             layer's fp32 output is also stored (store_tanh_x3's sink; rows that exist only) -- s1, s2; n1, n2, n3 (mlp)
//             or the per-neighbour e1, e2 at row b K + k and the mean m (mean_embed); o1, o2.  out is bitwise the rollout
//             kernel's.
//   backward  enc_mlp_bwd_x3_kernel, from dout [B, 2H] and the saves, per 64-agent tile:
//             phase A  dpre_ff = dout (1 - out^2) -> HBM (dW_ff's G operand), each row at its own power-of-two scale into
//                      ONE [64][2H + 8] split tile; then per part p, in the forward's order, dP_p = dpre_ff W_ff[:, pH ..]
//                      as mfma_layer_x3<H, 2H> on the packed transpose of that column block (the contraction over 2H, as
//                      the tail forward's layer 0): dpre_last = dP_p (1 - y_last^2) -> HBM, or dm = dP_p / K for the mean
//             phase B  the 2H tile is dead, an [64][H + 8] tile lies over it.  Per branch each lane reads dpre_last back
//                      at the accumulator positions it wrote (its own stores), stages it, multiplies by the packed W_2^T
//                      and the tanh derivative -> dpre_1 (the mlp branch once more: n3 -> n2 -> n1).  Layer 0 needs no dX.
//                      mean_embed: dm is held in the lane's accumulator-shaped registers and the forward's register sum
//                      runs in reverse, for k < K: dpre_e2,k = dm (1 - e2_k^2) -> stage -> W_n2^T -> (1 - e1_k^2) ->
//                      dpre_e1,k; lane l holds the same agents' columns for every k, nothing crosses a lane.
//             The weight gradients are qs_dw_x3_ld's, qs_attn_dw0_x3's and qs_colstats's (quadswarm_amd/enc_mlp_train.py).
//
// Backward work split, as policy_tail_bwd_x3_kernel: a block per tower WALKS the 64-agent tiles gridDim.x apart, so the
// column maxima of every pre-activation gradient (dW's column scales) are kept across its tiles -- the feed_forward's in
// the staging lanes' registers, the branches' seven H rows in LDS -- and written once per block.
//
// Backward LDS: the [64][2H + 8] hi / lo tile, RS [64] and RMX [4][64], the maxima CM [7][H].  H = 256: 133 120 + 1 280
// + 7 168 B, one block per CU; H = 128: 67 584 + 1 280 + 3 584 B, two blocks per CU by the launch bound.
//
// Zero gradient rows are the normal case (PPO's clip): a zero row takes scale 1 (row_scale) and contributes exact zeros;
// a non-finite value marks its column maximum +inf, as in the other backward kernels.
#pragma once
#include "qs_policy_enc.h"
#include "qs_policy_tail_train.h"   // colmax_fold_acc; qs_policy_train.h's staging helpers

namespace qs {
namespace pol {

struct EncTrains {
    qs_enc_train t[QS_ATTN_MAX_TOWERS];
};

// A weight pointer the optimiser cannot see through: the packed weights are the same for every tile a backward block walks
// (and for every neighbour k of the mean branch, in both directions), so their loads are loop-invariant and would be hoisted out of the loop -- a whole
// layer's weights in registers at once, spilled.  Laundered per iteration, each layer fetches its queue where it runs.
__device__ __forceinline__ const uint4* per_tile(const void* p) {
    asm volatile("" : "+s"(p));
    return reinterpret_cast<const uint4*>(p);
}

// ------------------------------------------------------------------------------------------------------------------
// forward with saves
// ------------------------------------------------------------------------------------------------------------------
// enc_layer0 / enc_layer (qs_policy_enc.h) with the fp32 rows also stored: row i of the tile at save[(row0 + i) rs + ro]
template <int H, int W>
__device__ __forceinline__ void enc_layer0_save(_Float16* src, _Float16* dst, const void* wp, const float* bias,
                                                f32x16 (&acc)[RT][Geo<H>::CT], int wave, int lane, float* save, long row0,
                                                long rs, long ro, int B) {
    mfma_layer_x3<H, W, true, false>(enc_tile(src, GeoX3<W>::LDH), reinterpret_cast<const uint4*>(wp), acc, wave, lane);
    store_tanh_x3<H>(enc_tile(dst, GeoX3<H>::LDH), acc, 1.f / (X3_SIN * X3_SW), wave, lane,
                     [&](int, int n0) { return lds4(bias + n0); },
                     [&](int i, int n0, float4 y) {
                         if (row0 + i < B) st4g(save + ((row0 + i) * rs + ro) * H + n0, y);
                     });
    __syncthreads();
}
template <int H>
__device__ __forceinline__ void enc_layer_save(_Float16* src, _Float16* dst, const void* wp, const float* bias,
                                               f32x16 (&acc)[RT][Geo<H>::CT], int wave, int lane, float* save, long row0,
                                               int B) {
    mfma_layer_x3<H>(enc_tile(src, GeoX3<H>::LDH), reinterpret_cast<const uint4*>(wp), acc, wave, lane);
    store_tanh_x3<H>(enc_tile(dst, GeoX3<H>::LDH), acc, 1.f / (X3_SX * X3_SW), wave, lane,
                     [&](int, int n0) { return lds4(bias + n0); },
                     [&](int i, int n0, float4 y) {
                         if (row0 + i < B) st4g(save + (row0 + i) * H + n0, y);
                     });
    __syncthreads();
}

template <int H, int NBR>
__global__ __launch_bounds__(NTHR, H == 256 ? 1 : 2) void enc_mlp_train_x3_kernel(const float* __restrict__ obs, int stride,
                                                                                 int so, int K, int nd, int od, int B,
                                                                                 EncTowers tw, EncTrains trs) {
    constexpr int LDH = GeoX3<H>::LDH, CT = Geo<H>::CT, TH = 2 * MROWS * LDH;
    static_assert(GeoX3<ENC_NBW>::LDH <= LDH, "every layer-0 input tile fits a tile's bytes");
    constexpr float iSS = 1.f / (X3_SX * X3_SW);
    extern __shared__ float4 smem4[];
    _Float16* th = reinterpret_cast<_Float16*>(smem4);
    _Float16 *ta = th, *tb = th + TH;   // ta: the tile that holds no part (the next gather's and layer's target)
    float* BI = reinterpret_cast<float*>(th + 2 * TH);   // b_s1, b_s2, b_n1, b_n2, b_n3, b_o1, b_o2, b_ff [2H]
    const qs_enc_tower& t = tw.t[blockIdx.y];
    const qs_enc_train& tr = trs.t[blockIdx.y];
    const long row0 = (long)blockIdx.x * MROWS;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int NP = 1 + (NBR != QS_ENC_NBR_NONE ? 1 : 0) + (od > 0 ? 1 : 0);

    for (int n = tid; n < H; n += NTHR) {
        BI[n] = t.b_s1[n];
        BI[H + n] = t.b_s2[n];
        if constexpr (NBR != QS_ENC_NBR_NONE) {
            BI[2 * H + n] = t.b_n1[n];
            BI[3 * H + n] = t.b_n2[n];
        }
        if constexpr (NBR == QS_ENC_NBR_MLP) BI[4 * H + n] = t.b_n3[n];
        if (od > 0) {
            BI[5 * H + n] = t.b_o1[n];
            BI[6 * H + n] = t.b_o2[n];
        }
        BI[7 * H + n] = t.b_ff[n];
        BI[8 * H + n] = t.b_ff[H + n];
    }
    auto swap = [&]() {
        _Float16* x = ta;
        ta = tb;
        tb = x;
    };

    f32x16 acc[RT][CT], accff[2][RT][CT];
    int p = 0;
    enc_gather0<ENC_SW>(enc_tile(ta, GeoX3<ENC_SW>::LDH), obs, stride, 0, so, B, row0, tid);
    __syncthreads();
    enc_layer0_save<H, ENC_SW>(ta, tb, t.w_s1p, BI, acc, wave, lane, tr.s1, row0, 1, 0, B);
    enc_layer_save<H>(tb, ta, t.w_s2p, BI + H, acc, wave, lane, tr.s2, row0, B);
    enc_ff<H, true>(ta, t.w_ffp, NP, p++, accff, wave, lane);
    swap();

    if constexpr (NBR == QS_ENC_NBR_MLP) {
        enc_gather0<ENC_NBW>(enc_tile(ta, GeoX3<ENC_NBW>::LDH), obs, stride, so, K * nd, B, row0, tid);
        __syncthreads();
        enc_layer0_save<H, ENC_NBW>(ta, tb, t.w_n1p, BI + 2 * H, acc, wave, lane, tr.n1, row0, 1, 0, B);
        enc_layer_save<H>(tb, ta, t.w_n2p, BI + 3 * H, acc, wave, lane, tr.n2, row0, B);
        enc_layer_save<H>(ta, tb, t.w_n3p, BI + 4 * H, acc, wave, lane, tr.n3, row0, B);
        enc_ff<H, false>(tb, t.w_ffp, NP, p++, accff, wave, lane);
    }
    if constexpr (NBR == QS_ENC_NBR_MEAN) {
        f32x16 sum[RT][CT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) sum[rt][c][r] = 0.f;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {   // the 64 agents' neighbour k; e1, e2 saved at row agent K + k
            enc_gather0<ENC_NDW>(enc_tile(ta, GeoX3<ENC_NDW>::LDH), obs, stride, so + k * nd, nd, B, row0, tid);
            __syncthreads();
            enc_layer0_save<H, ENC_NDW>(ta, tb, per_tile(t.w_n1p), BI + 2 * H, acc, wave, lane, tr.n1, row0, K, k, B);
            mfma_layer_x3<H>(enc_tile(tb, LDH), per_tile(t.w_n2p), acc, wave, lane);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const long agent = row0 + acc_i(rt, lane);
#pragma unroll
                for (int c = 0; c < CT; ++c)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int n0 = acc_n0<H>(wave, c, g, lane);
                        const float4 e = tanh_bias4(acc[rt][c], g, iSS, lds4(BI + 3 * H + n0));
                        if (agent < B) st4g(tr.n2 + (agent * K + k) * H + n0, e);
                        acc4_set(sum[rt][c], g, f4_add(acc4(sum[rt][c], g), e));
                    }
            }
        }
        const TileX3 P = enc_tile(ta, LDH);
        // the mean as sum (1 / K), rounded to fp32, THEN the tile's scale (qs_policy_enc.h on why)
        const float ik = 1.f / (float)K;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const long agent = row0 + acc_i(rt, lane);
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int n0 = acc_n0<H>(wave, c, g, lane);
                    const float4 m = f4_scale(acc4(sum[rt][c], g), ik);
                    if (agent < B) st4g(tr.m + agent * H + n0, m);
                    P.put4(acc_i(rt, lane), n0, f4_scale(m, X3_SX));   // (exact: 2^8)
                }
        }
        __syncthreads();
        enc_ff<H, false>(ta, t.w_ffp, NP, p++, accff, wave, lane);
        swap();
    }
    if (od > 0) {
        enc_gather0<ENC_OBW>(enc_tile(ta, GeoX3<ENC_OBW>::LDH), obs, stride, so + K * nd, od, B, row0, tid);
        __syncthreads();
        enc_layer0_save<H, ENC_OBW>(ta, tb, t.w_o1p, BI + 5 * H, acc, wave, lane, tr.o1, row0, 1, 0, B);
        enc_layer_save<H>(tb, ta, t.w_o2p, BI + 6 * H, acc, wave, lane, tr.o2, row0, B);
        enc_ff<H, false>(ta, t.w_ffp, NP, p++, accff, wave, lane);
    }

#pragma unroll
    for (int z = 0; z < 2; ++z)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const long agent = row0 + acc_i(rt, lane);
            if (agent >= B) continue;
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int n0 = acc_n0<H>(wave, c, g, lane);
                    st4g(t.out + (size_t)agent * (2 * H) + z * H + n0,
                         tanh_bias4(accff[z][rt][c], g, iSS, lds4(BI + (7 + z) * H + n0)));
                }
        }
}

// ------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------
constexpr int ENC_NCM = 7;   // CM rows: s1, s2, n1, n2, n3, o1, o2 (the colmax rows after the feed_forward's two)

template <int H>
constexpr size_t enc_bwd_lds_bytes() {
    return (size_t)(2 * MROWS * GeoX3<2 * H>::LDH) * 2 + (size_t)((1 + NWAVE) * MROWS + ENC_NCM * H) * 4;
}

// load_acc_rows (qs_policy_train.h) for rows rs apart: row i of the tile is src row (row0 + i) rs + ro
template <int H, typename Ok>
__device__ __forceinline__ void load_acc_rows_ld(const float* src, long row0, long rs, long ro, Ok okrow, int wave, int lane,
                                                 float4 (&v)[RT][Geo<H>::CT][4]) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int i = acc_i(rt, lane);
        const float* p = src + ((row0 + (okrow(i) ? i : 0)) * rs + ro) * H;
#pragma unroll
        for (int c = 0; c < Geo<H>::CT; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) v[rt][c][g] = ld4g(p + acc_n0<H>(wave, c, g, lane));
    }
}

// the last step of a chain: dpre = acc (RS / s_w) (1 - y^2) at the accumulator positions -> dst row (row0 + i) rs + ro,
// its column maxima folded into cm
template <int H, typename Ok>
__device__ __forceinline__ void enc_bwd_last(const f32x16 (&acc)[RT][Geo<H>::CT], const float4 (&y)[RT][Geo<H>::CT][4],
                                             const float* RS, float* dst, long row0, long rs, long ro, Ok okrow, float* cm,
                                             int wave, int lane) {
    constexpr int CT = Geo<H>::CT;
    float4 cma[CT][4];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int g = 0; g < 4; ++g) cma[c][g] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int i = acc_i(rt, lane);
        if (!okrow(i)) continue;
        const float sc = RS[i] * (1.f / X3_SW);
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 v = f4_dtanh(f4_scale(acc4(acc[rt][c], g), sc), y[rt][c][g]);
                st4g(dst + ((row0 + i) * rs + ro) * H + acc_n0<H>(wave, c, g, lane), v);
                cma[c][g] = absmax_acc4(cma[c][g], v);
            }
    }
    colmax_fold_acc<H>(cm, cma, wave, lane);
}

template <int H, int NBR>
__global__ __launch_bounds__(NTHR, H == 256 ? 1 : 2) void enc_mlp_bwd_x3_kernel(int K, int od, int B, EncTowers tw,
                                                                               EncTrains trs) {
    constexpr int LD2 = GeoX3<2 * H>::LDH, LDH = GeoX3<H>::LDH, CT = Geo<H>::CT;
    constexpr int NF = 2 * H / 256, BR = 4;         // float4 per lane of a 2H-wide row; rows per wave in flight
    constexpr float iSW = 1.f / X3_SW;
    constexpr size_t WBLK2 = (size_t)H * 2 * H / 4;   // uint4 per packed [H, 2H] block (hi + lo halves)
    extern __shared__ float4 smem4[];
    _Float16* gh = reinterpret_cast<_Float16*>(smem4);
    const TileX3 G2{gh, gh + MROWS * LD2, LD2};   // phase A: dpre_ff rows
    const TileX3 G{gh, gh + MROWS * LDH, LDH};    // phase B: over it
    float* RS = reinterpret_cast<float*>(gh + 2 * MROWS * LD2);   // 1 / s of the staged rows
    float* RMX = RS + MROWS;                                      // [NWAVE][MROWS] the waves' row maxima
    float* CM = RMX + NWAVE * MROWS;                              // [ENC_NCM][H] running column maxima
    const qs_enc_tower& t = tw.t[blockIdx.y];
    const qs_enc_train& tr = trs.t[blockIdx.y];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int e = tid; e < ENC_NCM * H; e += NTHR) CM[e] = 0.f;
    float4 cmff[NF];   // the feed_forward's maxima: the lane's columns 4 (lane + 64 f) .. + 3 over the wave's rows
#pragma unroll
    for (int f = 0; f < NF; ++f) cmff[f] = z4;

    const long n_tiles = ((long)B + MROWS - 1) / MROWS;
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long row0 = tile * MROWS;
        auto okrow = [&](int i) { return row0 + i < B; };
        __syncthreads();   // the previous tile's reads of the tile and RS (first tile: CM)
        const uint4* wfft = per_tile(tr.w_fft);

        // ---- phase A: dpre_ff = dout (1 - out^2), stored, row-scaled into the 2H tile (wave w: rows w, w + 4, ...)
#pragma unroll 1
        for (int r0 = wave; r0 < MROWS; r0 += NWAVE * BR) {
            float4 d[BR][NF], y[BR][NF];
#pragma unroll
            for (int u = 0; u < BR; ++u) {
                const long rr = row0 + (okrow(r0 + u * NWAVE) ? r0 + u * NWAVE : 0);   // unconditional loads
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    d[u][f] = ld4g(tr.dout + rr * (2 * H) + 4 * (lane + 64 * f));
                    y[u][f] = ld4g(t.out + rr * (2 * H) + 4 * (lane + 64 * f));
                }
            }
            float m[BR];
#pragma unroll
            for (int u = 0; u < BR; ++u) {
                const int r = r0 + u * NWAVE;
                m[u] = 0.f;
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    d[u][f] = okrow(r) ? f4_dtanh(d[u][f], y[u][f]) : z4;
                    if (okrow(r)) st4g(tr.dpre_ff + (row0 + r) * (2 * H) + 4 * (lane + 64 * f), d[u][f]);
                    cmff[f] = absmax_acc4(cmff[f], d[u][f]);
                    m[u] = fmaxf(m[u], absmax4(d[u][f]));
                }
            }
#pragma unroll
            for (int u = 0; u < BR; ++u) m[u] = wave_max(m[u]);
#pragma unroll
            for (int u = 0; u < BR; ++u) {
                const int r = r0 + u * NWAVE;
                const float s = row_scale(m[u]);
#pragma unroll
                for (int f = 0; f < NF; ++f) G2.put4(r, 4 * (lane + 64 * f), f4_scale(d[u][f], s));
                if (lane == 0) RS[r] = 1.f / s;
            }
        }
        __syncthreads();

        f32x16 acc[RT][CT];
        float4 aux[RT][CT][4];
        // part p: dP_p = dpre_ff W_ff[:, pH ..], then the last layer's tanh derivative (y_last in flight during the MFMAs)
        auto part_last = [&](int p, const float* ylast, float* dpre, float* cm) {
            load_acc_rows<H>(ylast, row0, okrow, wave, lane, aux);
            mfma_layer_x3<H, 2 * H>(G2, wfft + p * WBLK2, acc, wave, lane);
            enc_bwd_last<H>(acc, aux, RS, dpre, row0, 1, 0, okrow, cm, wave, lane);
        };
        int p = 0;
        part_last(p++, tr.s2, tr.dpre_s2, CM + 1 * H);
        if constexpr (NBR == QS_ENC_NBR_MLP) part_last(p++, tr.n3, tr.dpre_n3, CM + 4 * H);
        if constexpr (NBR == QS_ENC_NBR_MEAN) {   // dm = dP / K
            mfma_layer_x3<H, 2 * H>(G2, wfft + (p++) * WBLK2, acc, wave, lane);
            const float ik = 1.f / (float)K;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const int i = acc_i(rt, lane);
                if (!okrow(i)) continue;
                const float sc = RS[i] * iSW;
#pragma unroll
                for (int c = 0; c < CT; ++c)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        st4g(tr.dm + (row0 + i) * H + acc_n0<H>(wave, c, g, lane),
                             f4_scale(f4_scale(acc4(acc[rt][c], g), sc), ik));
            }
        }
        if (od > 0) part_last(p++, tr.o2, tr.dpre_o2, CM + 6 * H);

        // ---- phase B: the chains on the H tile.  One step: the gradient at the accumulator positions (src rows read back,
        // or acc itself through f) staged, times the packed W^T, times the previous layer's tanh derivative
        float4 cma[CT][4];
        auto readback = [&](int i, int, float4, float4 v) { return okrow(i) ? v : z4; };
        // dpre (own stores) -> tile -> dy = dpre W -> left in acc (scaled by s_i s_w), y_prev in aux
        auto step_from = [&](const float* dpre, const void* wt, const float* yprev) {
            load_acc_rows<H>(dpre, row0, okrow, wave, lane, aux);
            stage_acc_scaled<H>(G, acc, RS, RMX, wave, lane, aux, readback, cma);
            __syncthreads();
            load_acc_rows<H>(yprev, row0, okrow, wave, lane, aux);
            mfma_layer_x3<H>(G, per_tile(wt), acc, wave, lane);
        };
        step_from(tr.dpre_s2, tr.w_s2t, tr.s1);
        enc_bwd_last<H>(acc, aux, RS, tr.dpre_s1, row0, 1, 0, okrow, CM, wave, lane);
        if constexpr (NBR == QS_ENC_NBR_MLP) {
            step_from(tr.dpre_n3, tr.w_n3t, tr.n2);
            float* dp = tr.dpre_n2;
            stage_acc_scaled<H>(G, acc, RS, RMX, wave, lane, aux, [&](int i, int n0, float4 a, float4 y) {
                if (!okrow(i)) return z4;
                const float4 v = f4_dtanh(f4_scale(a, RS[i] * iSW), y);
                st4g(dp + (row0 + i) * H + n0, v);
                return v;
            }, cma);
            colmax_fold_acc<H>(CM + 3 * H, cma, wave, lane);
            __syncthreads();
            load_acc_rows<H>(tr.n1, row0, okrow, wave, lane, aux);
            mfma_layer_x3<H>(G, per_tile(tr.w_n2t), acc, wave, lane);
            enc_bwd_last<H>(acc, aux, RS, tr.dpre_n1, row0, 1, 0, okrow, CM + 2 * H, wave, lane);
        }
        if constexpr (NBR == QS_ENC_NBR_MEAN) {
            float4 dmr[RT][CT][4];   // dm at the lane's accumulator positions, for every k
            load_acc_rows<H>(tr.dm, row0, okrow, wave, lane, dmr);
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                load_acc_rows_ld<H>(tr.n2, row0, K, k, okrow, wave, lane, aux);   // e2_k
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int c = 0; c < CT; ++c)
#pragma unroll
                        for (int g = 0; g < 4; ++g) acc4_set(acc[rt][c], g, dmr[rt][c][g]);
                float* dp = tr.dpre_n2;
                stage_acc_scaled<H>(G, acc, RS, RMX, wave, lane, aux, [&](int i, int n0, float4 a, float4 e2) {
                    if (!okrow(i)) return z4;
                    const float4 v = f4_dtanh(a, e2);
                    st4g(dp + ((row0 + i) * K + k) * H + n0, v);
                    return v;
                }, cma);
                colmax_fold_acc<H>(CM + 3 * H, cma, wave, lane);
                __syncthreads();
                load_acc_rows_ld<H>(tr.n1, row0, K, k, okrow, wave, lane, aux);   // e1_k
                mfma_layer_x3<H>(G, per_tile(tr.w_n2t), acc, wave, lane);
                enc_bwd_last<H>(acc, aux, RS, tr.dpre_n1, row0, K, k, okrow, CM + 2 * H, wave, lane);
            }
        }
        if (od > 0) {
            step_from(tr.dpre_o2, tr.w_o2t, tr.o1);
            enc_bwd_last<H>(acc, aux, RS, tr.dpre_o1, row0, 1, 0, okrow, CM + 5 * H, wave, lane);
        }
    }

    // the block's maxima, once: colmax [2 + ENC_NCM][gridDim.x][H]; the feed_forward's through the (dead) tile's bytes
    __syncthreads();   // the last tile's tile reads and CM folds
    float* SCR = reinterpret_cast<float*>(smem4);   // [NWAVE][2H]
#pragma unroll
    for (int f = 0; f < NF; ++f) *reinterpret_cast<float4*>(SCR + wave * (2 * H) + 4 * (lane + 64 * f)) = cmff[f];
    __syncthreads();
    for (int n = tid; n < 2 * H; n += NTHR)
        tr.colmax[((size_t)(n / H) * gridDim.x + blockIdx.x) * H + n % H] =
            fmaxf(fmaxf(SCR[n], SCR[2 * H + n]), fmaxf(SCR[4 * H + n], SCR[6 * H + n]));
    for (int e = tid; e < ENC_NCM * H; e += NTHR)
        tr.colmax[((size_t)(2 + e / H) * gridDim.x + blockIdx.x) * H + e % H] = CM[e];
}

}  // namespace pol
}  // namespace qs
