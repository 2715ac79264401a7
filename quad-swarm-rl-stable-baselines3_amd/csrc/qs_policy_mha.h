// qs_policy_mha.h -- fused no-grad forward of the obstacle policies' multi-head attention encoder on the split-f16
// matrix cores (precision x3 only; qs_policy_x3.h's tile, layer and scales).
//
// QuadMultiHeadAttentionEncoder (swarm_rl/models/quad_multi_model.py:125-200) up to its LayerNorm, per agent:
//   x_0 = tanh(tanh(nbr W_n1^T + b_n1) W_n2^T + b_n2)       neighbor_embed_layer on the whole [K nd] neighbour block
//   x_1 = tanh(tanh(obst W_o1^T + b_o1) W_o2^T + b_o2)      obstacle_embed_layer
//   per head h < 4 (attention_layer.py:10-54, d_k = d_v = H):
//     q_t = x_t Wq_h^T, k_t = x_t Wk_h^T, v_t = x_t Wv_h^T,  a[t][.] = softmax_u(q_t . k_u / sqrt(H))
//     ctx_t = a[t][0] v_0 + a[t][1] v_1
//   y_t = sum_h ctx_t^h Wfc[:, hH:(h+1)H]^T + x_t,  out[agent][t H ..] = LayerNorm(y_t) gamma + beta   (eps 1e-6)
// i.e. attn_embed.view(batch, -1), [B, 2H]: 18 H x H GEMMs per token row with nothing but the raw observations read
// and the normalised tokens written.
//
// Row split: a block owns 32 agents as 64 rows, rows 0..31 their neighbour tokens and rows 32..63 the same agents'
// obstacle tokens.  MFMA row tile rt is therefore token rt, and in the accumulator layout (qs_policy.h acc_i /
// acc_n0) lane l holds BOTH tokens of agent l & 31 at the same output columns in acc[0] and acc[1]: the score dots,
// the softmax and the context mix never cross a lane, apart from the column reduction of the four scores.
//
// LDS: X (the tokens, split f16 at X3_SX, kept for all four heads and the residual) and C (one head's context at
// X3_SC; layer 0's gathered input before head 0, the fp32 residual rows after head 3), [64][H + 8] halves twice each:
// 2 x 67 584 B at H = 256 plus a 6 H float table and the score partials -- 143 KB, one block per CU; 75 KB at
// H = 128, two blocks per CU.  Registers: the Y, Q (then V) and K accumulators live together, 3 x 64 at H = 256.
#pragma once
#include "qs_policy_x3.h"

namespace qs {
namespace pol {

constexpr int MHA_HEADS = 4;
constexpr int MHA_AG = MROWS / 2;     // agents per block
constexpr int MHA_NBW = 64;           // layer 0 columns [0, 64): the neighbour block (K nd <= 64), zero padded
constexpr int MHA_OBW = 16;           // layer 0 columns [64, 80): the obstacle values (<= 16), zero padded
constexpr int MHA_KD0 = MHA_NBW + MHA_OBW;
constexpr float X3_SC = 16.f;         // context scale: |ctx| <= max_row |w_vs|_1 (|x| <= 1), checked < 65504 / 16 at refresh

struct MhaTowers {
    qs_mha_tower t[QS_ATTN_MAX_TOWERS];
};

// mfma_layer_x3 with one packed weight per 32-row tile (row tile rt contracts with Wp[rt]): the same MFMAs, twice the
// weight loads -- the two tokens' second embedding layers in one pass over the tile, no zero-widened contraction.
template <int H, bool PIN = true>
__device__ __forceinline__ void mfma_layer_x3_rt(const TileX3& X, const uint4* const (&Wp)[RT],
                                                 f32x16 (&acc)[RT][Geo<H>::CT], int wave, int lane) {
    constexpr int CT = Geo<H>::CT, S = GeoX3<H>::S;
    WQueue<H> q[RT];
    const uint4* wb[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        q[rt] = mfma_prefetch_x3<H>(Wp[rt], wave, lane);
        wb[rt] = wlane_base<H>(Wp[rt], wave, lane);
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[rt][c][r] = 0.f;
    }
    const int aoff = (lane & 31) * X.ld + (lane >> 5) * 8;
    auto wld = [&](int rt, int c, int s, int part) { return wb[rt][((size_t)(c * S + s) * 64) * 2 + part]; };
    auto ald = [&](const _Float16* t, int rt, int s) {
        return *reinterpret_cast<const f16x8*>(t + aoff + rt * 32 * X.ld + 16 * s);
    };
    f16x8 ahn[RT], aln[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        ahn[rt] = ald(X.h, rt, 0);
        aln[rt] = ald(X.l, rt, 0);
    }
    for (int s = 0; s < S; ++s) {
        f16x8 ah[RT], al[RT], bh[RT][CT], bl[RT][CT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
            for (int c = 0; c < CT; ++c) {   // weights: two steps in flight ahead of the MFMAs
                bh[rt][c] = __builtin_bit_cast(f16x8, q[rt].bh0[c]);
                bl[rt][c] = __builtin_bit_cast(f16x8, q[rt].bl0[c]);
                q[rt].bh0[c] = q[rt].bh1[c];
                q[rt].bl0[c] = q[rt].bl1[c];
                if (s + 2 < S) {
                    q[rt].bh1[c] = wld(rt, c, s + 2, 0);
                    q[rt].bl1[c] = wld(rt, c, s + 2, 1);
                }
            }
            ah[rt] = ahn[rt];   // activations: one step ahead
            al[rt] = aln[rt];
            if (s + 1 < S) {
                ahn[rt] = ald(X.h, rt, s + 1);
                aln[rt] = ald(X.l, rt, s + 1);
            }
        }
        if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);   // (mfma_layer_x3: keep the queue where it is written)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                acc[rt][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[rt][c], ah[rt], acc[rt][c], 0, 0, 0);
                acc[rt][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl[rt][c], ah[rt], acc[rt][c], 0, 0, 0);
                acc[rt][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[rt][c], al[rt], acc[rt][c], 0, 0, 0);
            }
        if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
    }
}

// Layer 0's input tile [64][80] at X3_SIN: token-0 rows carry the agent's neighbour block in columns [0, nbw) and
// token-1 rows its obstacle values in columns [64, 64 + od); everything else is zero.  The loads are unconditional and
// back to back (qs_policy.h gather_rows0): a column past the data reads the agent's word 0 and a row past B reads
// obs[0], both zeroed by a product.
__device__ __forceinline__ void mha_gather0(const TileX3& X0, const float* __restrict__ obs, int stride, int so, int nbw,
                                            int od, int B, long ag0, int tid) {
    constexpr int NN = MHA_AG * MHA_NBW / NTHR, NO = MHA_AG * MHA_OBW / NTHR;
    float vn[NN], vo[NO];
#pragma unroll
    for (int u = 0; u < NN; ++u) {
        const int e = tid + u * NTHR, r = e / MHA_NBW, c = e - r * MHA_NBW;
        const bool ok = ag0 + r < B && c < nbw;
        vn[u] = obs[(ag0 + r < B ? (size_t)(ag0 + r) * stride : 0) + (ok ? so + c : 0)] * (ok ? X3_SIN : 0.f);
    }
#pragma unroll
    for (int u = 0; u < NO; ++u) {
        const int e = tid + u * NTHR, r = e / MHA_OBW, c = e - r * MHA_OBW;
        const bool ok = ag0 + r < B && c < od;
        vo[u] = obs[(ag0 + r < B ? (size_t)(ag0 + r) * stride : 0) + (ok ? so + nbw + c : 0)] * (ok ? X3_SIN : 0.f);
    }
#pragma unroll
    for (int u = 0; u < NN; ++u) {
        const int e = tid + u * NTHR, r = e / MHA_NBW, c = e - r * MHA_NBW;
        X0.put(r, c, vn[u]);
        X0.put(MHA_AG + r, c, 0.f);
    }
#pragma unroll
    for (int u = 0; u < NO; ++u) {
        const int e = tid + u * NTHR, r = e / MHA_OBW, c = e - r * MHA_OBW;
        X0.put(r, MHA_NBW + c, 0.f);
        X0.put(MHA_AG + r, MHA_NBW + c, vo[u]);
    }
}

template <int H>
constexpr size_t mha_lds_bytes() {
    return (size_t)(4 * MROWS * GeoX3<H>::LDH) * 2 + (size_t)(6 * H + NWAVE * 4 * MHA_AG) * 4;
}

// raw observations -> the post-LayerNorm tokens out [B, 2H] of one tower (blockIdx.y), 32 agents per block
template <int H>
__global__ __launch_bounds__(NTHR, H == 256 ? 1 : 2) void mha_encoder_x3_kernel(const float* __restrict__ obs, int stride,
                                                                               int so, int nbw, int od, int B,
                                                                               MhaTowers tw) {
    constexpr int LDH = GeoX3<H>::LDH, LD0 = GeoX3<MHA_KD0>::LDH, CT = Geo<H>::CT, LDF = H + 4;
    static_assert(2 * MROWS * LD0 <= 2 * MROWS * LDH, "layer 0's input tile fits the context tile's bytes");
    static_assert(MROWS * LDF * 4 <= 2 * MROWS * LDH * 2, "the fp32 residual tile fits the context tile's bytes");
    extern __shared__ float4 smem4[];
    _Float16* xh = reinterpret_cast<_Float16*>(smem4);
    const TileX3 X{xh, xh + MROWS * LDH, LDH};
    _Float16* ch = xh + 2 * MROWS * LDH;
    const TileX3 C{ch, ch + MROWS * LDH, LDH};
    const TileX3 X0{ch, ch + MROWS * LD0, LD0};       // over C: dead before head 0 writes its context
    float* F = reinterpret_cast<float*>(ch);          // over C: the residual rows, after head 3's last read
    float* BI = reinterpret_cast<float*>(ch + 2 * MROWS * LDH);   // b_n1, b_o1, b_n2, b_o2, gamma, beta
    float* SCP = BI + 6 * H;                          // [wave][t][u][agent]: the waves' score partials
    const qs_mha_tower& t = tw.t[blockIdx.y];
    const long ag0 = (long)blockIdx.x * MHA_AG;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, ag = lane & 31;
    constexpr size_t WBLK = (size_t)H * H * 2 * 2 / 16;   // uint4 per packed H x H block
    constexpr float iSS = 1.f / (X3_SX * X3_SW);

    for (int n = tid; n < H; n += NTHR) {
        BI[n] = t.b_n1[n];
        BI[H + n] = t.b_o1[n];
        BI[2 * H + n] = t.b_n2[n];
        BI[3 * H + n] = t.b_o2[n];
        BI[4 * H + n] = t.ln_g[n];
        BI[5 * H + n] = t.ln_b[n];
    }
    mha_gather0(X0, obs, stride, so, nbw, od, B, ag0, tid);
    __syncthreads();

    // the two embedding MLPs: layer 0 on the packed [W_n1 | W_o1] (the other token's columns are zero in each row),
    // layer 1 with one weight per row tile; the bias by row half
    f32x16 acc[RT][CT];
    mfma_layer_x3<H, MHA_KD0, true, false>(X0, reinterpret_cast<const uint4*>(t.w_e1p), acc, wave, lane);
    store_tanh_x3<H>(X, acc, 1.f / (X3_SIN * X3_SW), wave, lane, [&](int i, int n0) { return lds4(BI + (i >> 5) * H + n0); });
    __syncthreads();
    {
        const uint4* const w2[RT] = {reinterpret_cast<const uint4*>(t.w_n2p), reinterpret_cast<const uint4*>(t.w_o2p)};
        mfma_layer_x3_rt<H>(X, w2, acc, wave, lane);
    }
    __syncthreads();   // every wave has read the tile
    store_tanh_x3<H>(X, acc, iSS, wave, lane, [&](int i, int n0) { return lds4(BI + (2 + (i >> 5)) * H + n0); });
    __syncthreads();

    // the heads: Y accumulates sum_h ctx^h Wfc_h^T at scale X3_SC X3_SW
    f32x16 accy[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) accy[rt][c][r] = 0.f;
    const float sc = iSS * iSS / sqrtf((float)H);   // the two projections' scales and the temperature
#pragma unroll 1
    for (int h = 0; h < MHA_HEADS; ++h) {
        f32x16 acck[RT][CT];
        mfma_layer_x3<H>(X, reinterpret_cast<const uint4*>(t.w_qp) + h * WBLK, acc, wave, lane);
        mfma_layer_x3<H>(X, reinterpret_cast<const uint4*>(t.w_kp) + h * WBLK, acck, wave, lane);
        // q_t . k_u over this lane's columns, then the other lane half's (same agent, other columns); the four waves'
        // column ranges are added after the barrier, in wave order
        float p[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int tq = 0; tq < 2; ++tq)
#pragma unroll
                    for (int u = 0; u < 2; ++u) p[tq][u] = fmaf(acc[tq][c][r], acck[u][c][r], p[tq][u]);
#pragma unroll
        for (int tq = 0; tq < 2; ++tq)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                p[tq][u] += __shfl_xor(p[tq][u], 32);
                if (lane < 32) SCP[((wave * 2 + tq) * 2 + u) * MHA_AG + ag] = p[tq][u];
            }
        mfma_layer_x3<H>(X, reinterpret_cast<const uint4*>(t.w_vp) + h * WBLK, acc, wave, lane);   // V over Q
        __syncthreads();   // the partials are complete; every wave is past the previous head's reads of C
        float a[2][2];
#pragma unroll
        for (int tq = 0; tq < 2; ++tq) {   // every wave, redundantly: its lanes' own agents
            float s[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float* pp = SCP + (tq * 2 + u) * MHA_AG + ag;
                s[u] = ((pp[0] + pp[4 * MHA_AG]) + (pp[8 * MHA_AG] + pp[12 * MHA_AG])) * sc;
            }
            const float m = fmaxf(s[0], s[1]);
            const float e0 = expf(s[0] - m), e1 = expf(s[1] - m), d = e0 + e1;
            a[tq][0] = e0 / d;
            a[tq][1] = e1 / d;
        }
#pragma unroll
        for (int tq = 0; tq < 2; ++tq)
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 v0 = acc4(acc[0][c], g), v1 = acc4(acc[1][c], g);
                    const float4 cx = make_float4(a[tq][0] * v0.x + a[tq][1] * v1.x, a[tq][0] * v0.y + a[tq][1] * v1.y,
                                                  a[tq][0] * v0.z + a[tq][1] * v1.z, a[tq][0] * v0.w + a[tq][1] * v1.w);
                    C.put4(acc_i(tq, lane), acc_n0<H>(wave, c, g, lane), f4_scale(cx, X3_SC * iSS));   // (exact: 2^-12)
                }
        __syncthreads();   // C is complete (and every wave has read the partials)
        mfma_layer_x3<H, H, false>(C, reinterpret_cast<const uint4*>(t.w_fcp) + h * WBLK, accy, wave, lane);
    }
    __syncthreads();   // every wave has read C

    // y = Y + x in fp32 rows over C's bytes, then the LayerNorm: wave w its rows [16 w, 16 w + 16), a row's H / 4
    // float4 on as many lanes (two rows per pass at H = 128), mean first, then the centred sum of squares
    constexpr float iSY = 1.f / (X3_SC * X3_SW), iSX = 1.f / X3_SX;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int i = acc_i(rt, lane);
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n0 = acc_n0<H>(wave, c, g, lane);
                const float4 y = acc4(accy[rt][c], g);
                *reinterpret_cast<float4*>(F + i * LDF + n0) =
                    make_float4(fmaf(y.x, iSY, X.get(i, n0) * iSX), fmaf(y.y, iSY, X.get(i, n0 + 1) * iSX),
                                fmaf(y.z, iSY, X.get(i, n0 + 2) * iSX), fmaf(y.w, iSY, X.get(i, n0 + 3) * iSX));
            }
    }
    __syncthreads();
    constexpr int LPR = H / 4, RPP = 64 / LPR;   // lanes per row, rows per pass
    const int c4 = lane % LPR;
    const float4 gm = lds4(BI + 4 * H + 4 * c4), bt = lds4(BI + 5 * H + 4 * c4);
    for (int r = 0; r < MROWS / NWAVE; r += RPP) {
        const int i = wave * (MROWS / NWAVE) + r + lane / LPR;
        const float4 v = lds4(F + i * LDF + 4 * c4);
        float s = (v.x + v.y) + (v.z + v.w);
#pragma unroll
        for (int m = LPR / 2; m >= 1; m >>= 1) s += __shfl_xor(s, m);
        const float mean = s * (1.f / H);
        const float4 d = make_float4(v.x - mean, v.y - mean, v.z - mean, v.w - mean);
        float q = (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
#pragma unroll
        for (int m = LPR / 2; m >= 1; m >>= 1) q += __shfl_xor(q, m);
        const float rs = 1.f / sqrtf(q * (1.f / H) + 1e-6f);
        const long agent = ag0 + (i & 31);
        if (agent < B)
            st4g(t.out + (size_t)agent * (2 * H) + (size_t)(i >> 5) * H + 4 * c4,
                 make_float4(fmaf(d.x * rs, gm.x, bt.x), fmaf(d.y * rs, gm.y, bt.y), fmaf(d.z * rs, gm.z, bt.z),
                             fmaf(d.w * rs, gm.w, bt.w)));
    }
}

}  // namespace pol
}  // namespace qs
