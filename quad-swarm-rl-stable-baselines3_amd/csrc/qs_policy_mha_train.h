// qs_policy_mha_train.h -- the PPO update's side of the multi-head attention encoder (qs_policy_mha.h) on the split-f16
// matrix cores: the forward with the activations the backward needs saved, and the backward's data gradient.
//
// Forward (mha_encoder_train_x3_kernel): the rollout kernel's phase sequence, written out a second time so that the
// rollout instance keeps the code it has (a shared body put spills into the other family's rollout
// kernel), plus the stores of x1 (layer-1 tanh outputs), X (the tokens), the 16 softmax weights per agent, the
// LayerNorm's normalised rows and 1 / sigma.  Q, K, V and the per-head contexts are not saved.
//
// Backward (mha_bwd_x3_kernel), per agent with t, u the two tokens, s = the saved softmax weights of head h:
//   dy_t   = (g_t - mean(g_t) - xhat_t mean(g_t xhat_t)) / sigma_t,   g_t = dout_t gamma        LayerNorm; dX = dy
//   dctx_t = dy_t Wfc_h,  v_u = x_u Wv_h^T (recomputed),  da[t][u] = dctx_t . v_u
//   dv_u   = sum_t s[t][u] dctx_t,   ds[t][u] = s[t][u] (da[t][u] - sum_u' s[t][u'] da[t][u']) / sqrt(H)
//   q, k recomputed,  dq_t = sum_u ds[t][u] k_u,  dk_u = sum_t ds[t][u] q_t
//   dX    += dq Wq_h + dk Wk_h + dv Wv_h
//   G_h[u] = sum_t s[t][u] dy_t,  R_h[t] = sum_u ds[t][u] x_u      the row mixes of the attention weight gradients:
//            E_h = G_h^T X and S_h = R_h^T X (qs_dw_x3_ld, A = X with |x| <= 1) give dWfc_h = E_h Wv_h^T,
//            dWv_h = Wfc_h^T E_h, dWq_h = Wk_h S_h, dWk_h = Wq_h S_h^T on the host (mha_train.py)
//   dpre2  = dX (1 - X^2),  dx1 = dpre2 W_{n2|o2} (one W^T per row tile),  dpre1 = dx1 (1 - x1^2)
//
// Work split: the forward's -- 32 agents per block as 64 rows, row tile rt = token rt, so a lane holds both tokens of
// its agent at the same columns in acc[0] / acc[1]: every per-agent mix above is lane-local, and only the four da
// dots cross lanes (the other lane half, then the four waves' column ranges through LDS, like the forward's scores).
// LDS: the token tile X (split f16 at X3_SX, kept for every recomputation) and one gradient tile T whose rows carry
// their own power-of-two scales (qs_policy_train.h row_scale): dy is re-staged into T at each head, then dv, dq and dk
// pass through it in turn.  Registers: two accumulator sets (dctx / V, then Q / K, then a staged gradient's product)
// and the weight queue; dy and the running dX are parked in HBM between their uses (in the dpre2 / dpre1 buffers, which
// the last phase overwrites; each lane reads back only what it stored) -- resident in registers they put spills into
// both instances.
#pragma once
#include "qs_policy_mha.h"
#define QS_TRAIN_STAGING_ONLY 1   // row_scale, the DPP reductions, colmax_store_acc
#include "qs_policy_train.h"

namespace qs {
namespace pol {

struct MhaTrains {
    qs_mha_train t[QS_ATTN_MAX_TOWERS];
};

// block row i (agent ag0 + (i & 31), token i >> 5) -> its row of a [B, 2, H] array; agent 0 stands in past B
__device__ __forceinline__ size_t mha_row(long ag0, int i, int B) {
    const long a = ag0 + (i & 31);
    return (size_t)(a < B ? a : 0) * 2 + (size_t)(i >> 5);
}

// ------------------------------------------------------------------------------------------------------------------
// forward with saves: mha_encoder_x3_kernel's phases and arithmetic (out is bitwise the rollout kernel's)
// ------------------------------------------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(NTHR, H == 256 ? 1 : 2) void mha_encoder_train_x3_kernel(const float* __restrict__ obs,
                                                                                     int stride, int so, int nbw, int od,
                                                                                     int B, MhaTowers tw, MhaTrains trs) {
    constexpr int LDH = GeoX3<H>::LDH, LD0 = GeoX3<MHA_KD0>::LDH, CT = Geo<H>::CT, LDF = H + 4;
    extern __shared__ float4 smem4[];
    _Float16* xh = reinterpret_cast<_Float16*>(smem4);
    const TileX3 X{xh, xh + MROWS * LDH, LDH};
    _Float16* ch = xh + 2 * MROWS * LDH;
    const TileX3 C{ch, ch + MROWS * LDH, LDH};
    const TileX3 X0{ch, ch + MROWS * LD0, LD0};
    float* F = reinterpret_cast<float*>(ch);
    float* BI = reinterpret_cast<float*>(ch + 2 * MROWS * LDH);
    float* SCP = BI + 6 * H;
    const qs_mha_tower& t = tw.t[blockIdx.y];
    const qs_mha_train& tr = trs.t[blockIdx.y];
    const long ag0 = (long)blockIdx.x * MHA_AG;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, ag = lane & 31;
    constexpr size_t WBLK = (size_t)H * H * 2 * 2 / 16;
    constexpr float iSS = 1.f / (X3_SX * X3_SW);
    auto save = [&](float* dst, int i, int n0, float4 y) {   // the fp32 tanh values of the block's rows that exist
        if (ag0 + (i & 31) < B) st4g(dst + mha_row(ag0, i, B) * H + n0, y);
    };

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

    f32x16 acc[RT][CT];
    mfma_layer_x3<H, MHA_KD0, true, false>(X0, reinterpret_cast<const uint4*>(t.w_e1p), acc, wave, lane);
    store_tanh_x3<H>(X, acc, 1.f / (X3_SIN * X3_SW), wave, lane, [&](int i, int n0) { return lds4(BI + (i >> 5) * H + n0); },
                     [&](int i, int n0, float4 y) { save(tr.x1, i, n0, y); });
    __syncthreads();
    {
        const uint4* const w2[RT] = {reinterpret_cast<const uint4*>(t.w_n2p), reinterpret_cast<const uint4*>(t.w_o2p)};
        mfma_layer_x3_rt<H>(X, w2, acc, wave, lane);
    }
    __syncthreads();
    store_tanh_x3<H>(X, acc, iSS, wave, lane, [&](int i, int n0) { return lds4(BI + (2 + (i >> 5)) * H + n0); },
                     [&](int i, int n0, float4 y) { save(tr.x, i, n0, y); });
    __syncthreads();

    f32x16 accy[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) accy[rt][c][r] = 0.f;
    const float sc = iSS * iSS / sqrtf((float)H);
#pragma unroll 1
    for (int h = 0; h < MHA_HEADS; ++h) {
        f32x16 acck[RT][CT];
        mfma_layer_x3<H>(X, reinterpret_cast<const uint4*>(t.w_qp) + h * WBLK, acc, wave, lane);
        mfma_layer_x3<H>(X, reinterpret_cast<const uint4*>(t.w_kp) + h * WBLK, acck, wave, lane);
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
        mfma_layer_x3<H>(X, reinterpret_cast<const uint4*>(t.w_vp) + h * WBLK, acc, wave, lane);
        __syncthreads();
        float a[2][2];
#pragma unroll
        for (int tq = 0; tq < 2; ++tq) {
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
        if (wave == 0 && lane < 32 && ag0 + ag < B)   // s[h][t][u] of the lane's agent
            st4g(tr.sm + ((size_t)(ag0 + ag) * MHA_HEADS + h) * 4, make_float4(a[0][0], a[0][1], a[1][0], a[1][1]));
#pragma unroll
        for (int tq = 0; tq < 2; ++tq)
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 v0 = acc4(acc[0][c], g), v1 = acc4(acc[1][c], g);
                    const float4 cx = make_float4(a[tq][0] * v0.x + a[tq][1] * v1.x, a[tq][0] * v0.y + a[tq][1] * v1.y,
                                                  a[tq][0] * v0.z + a[tq][1] * v1.z, a[tq][0] * v0.w + a[tq][1] * v1.w);
                    C.put4(acc_i(tq, lane), acc_n0<H>(wave, c, g, lane), f4_scale(cx, X3_SC * iSS));
                }
        __syncthreads();
        mfma_layer_x3<H, H, false>(C, reinterpret_cast<const uint4*>(t.w_fcp) + h * WBLK, accy, wave, lane);
    }
    __syncthreads();

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
    constexpr int LPR = H / 4, RPP = 64 / LPR;
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
        if (agent < B) {
            const float4 xn = make_float4(d.x * rs, d.y * rs, d.z * rs, d.w * rs);
            const size_t row = (size_t)agent * 2 + (size_t)(i >> 5);
            st4g(t.out + row * H + 4 * c4,
                 make_float4(fmaf(xn.x, gm.x, bt.x), fmaf(xn.y, gm.y, bt.y), fmaf(xn.z, gm.z, bt.z), fmaf(xn.w, gm.w, bt.w)));
            st4g(tr.xhat + row * H + 4 * c4, xn);
            if (c4 == 0) tr.rsig[row] = rs;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------
template <int H>
constexpr size_t mha_bwd_lds_bytes() {   // X and T tiles + gamma, SY, RSY, RS (MROWS each), RMX, the da partials
    return (size_t)(4 * MROWS * GeoX3<H>::LDH) * 2 + (size_t)(H + 3 * MROWS + NWAVE * MROWS + NWAVE * 4 * MHA_AG) * 4;
}

__device__ __forceinline__ float4 tile_get4(const TileX3& X, int i, int n0) {   // s x of four consecutive columns
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    const f16x4 a = *reinterpret_cast<const f16x4*>(X.h + i * X.ld + n0);
    const f16x4 b = *reinterpret_cast<const f16x4*>(X.l + i * X.ld + n0);
    return make_float4((float)a[0] + (float)b[0], (float)a[1] + (float)b[1], (float)a[2] + (float)b[2],
                       (float)a[3] + (float)b[3]);
}

// Gradient rows held in accumulator layout -> the tile T, each row at its own power-of-two scale (its maximum over the
// four waves' column ranges through RMX), RS[i] = 1 / scale.  The first barrier also separates the previous layer's
// reads of T (and of RS) from the overwrite; the second completes the tile.
template <int H>
__device__ __forceinline__ void mha_stage_acc(const TileX3& T, const f32x16 (&acc)[RT][Geo<H>::CT], float* RS, float* RMX,
                                              int wave, int lane) {
    constexpr int CT = Geo<H>::CT;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        float m = 0.f;
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) m = fmaxf(m, fabsf(acc[rt][c][r]));
        m = fmaxf(m, __shfl_xor(m, 32));
        if (lane < 32) RMX[wave * MROWS + acc_i(rt, lane)] = m;
    }
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int i = acc_i(rt, lane);
        const float s = row_scale(fmaxf(fmaxf(RMX[i], RMX[MROWS + i]), fmaxf(RMX[2 * MROWS + i], RMX[3 * MROWS + i])));
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) T.put4(i, acc_n0<H>(wave, c, g, lane), f4_scale(acc4(acc[rt][c], g), s));
        if (wave == 0 && lane < 32) RS[i] = 1.f / s;
    }
    __syncthreads();
}

// the lane's accumulator positions of a [B, 2, H] array it alone reads and writes (dy and the running dX, parked in
// HBM between their uses): 0 on rows past B
template <int H>
__device__ __forceinline__ float4 mha_ld_own(const float* src, long ag0, int B, int i, int n0) {
    const float4 v = ld4g(src + mha_row(ag0, i, B) * H + n0);
    return ag0 + (i & 31) < B ? v : make_float4(0.f, 0.f, 0.f, 0.f);
}
// dX += P / (row scale, weight scale) for a product P of the tile staged by mha_stage_acc
template <int H>
__device__ __forceinline__ void mha_add_rows(float* dX, const f32x16 (&P)[RT][Geo<H>::CT], const float* RS,
                                             long ag0, int B, int wave, int lane) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int i = acc_i(rt, lane);
        if (ag0 + (i & 31) >= B) continue;
        const float s = RS[i] * (1.f / X3_SW);
        float* row = dX + mha_row(ag0, i, B) * H;
#pragma unroll
        for (int c = 0; c < Geo<H>::CT; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float* q = row + acc_n0<H>(wave, c, g, lane);
                const float4 o = ld4g(q), v = acc4(P[rt][c], g);
                st4g(q, make_float4(fmaf(v.x, s, o.x), fmaf(v.y, s, o.y), fmaf(v.z, s, o.z), fmaf(v.w, s, o.w)));
            }
    }
}

// f(rt, c, g, i, n0) -> float4 at the lane's accumulator positions (0 on rows past B) to dst [B, 2, H], with the
// block's column maxima: one row of maxima over both tokens at cm, or (PER_TOKEN) token t's at cm + t * cm_stride
template <int H, bool PER_TOKEN, typename F>
__device__ __forceinline__ void mha_store_rows(float* dst, float* cm, size_t cm_stride, long ag0, int B,
                                               int wave, int lane, F f) {
    constexpr int CT = Geo<H>::CT;
    float4 m[CT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        if (rt == 0 || PER_TOKEN) {
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int g = 0; g < 4; ++g) m[c][g] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const int i = acc_i(rt, lane);
        const bool ok = ag0 + (i & 31) < B;
        float* row = dst + mha_row(ag0, i, B) * H;
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n0 = acc_n0<H>(wave, c, g, lane);
                const float4 v = f(rt, c, g, i, n0);
                if (ok) st4g(row + n0, v);
                m[c][g] = absmax_acc4(m[c][g], v);
            }
        if (PER_TOKEN) colmax_store_acc<H>(cm + rt * cm_stride, m, wave, lane);
    }
    if (!PER_TOKEN) colmax_store_acc<H>(cm, m, wave, lane);
}

template <int H>
__global__ __launch_bounds__(NTHR, H == 256 ? 1 : 2) void mha_bwd_x3_kernel(int B, MhaTowers tw, MhaTrains trs) {
    constexpr int LDH = GeoX3<H>::LDH, CT = Geo<H>::CT, LDF = H + 4;
    static_assert(MROWS * LDF * 4 <= 2 * MROWS * LDH * 2, "the fp32 dy rows fit the gradient tile's bytes");
    extern __shared__ float4 smem4[];
    _Float16* xh = reinterpret_cast<_Float16*>(smem4);
    const TileX3 X{xh, xh + MROWS * LDH, LDH};
    _Float16* th = xh + 2 * MROWS * LDH;
    const TileX3 T{th, th + MROWS * LDH, LDH};
    float* F = reinterpret_cast<float*>(th);          // over T: dy's fp32 rows between the LayerNorm and the first staging
    float* GM = reinterpret_cast<float*>(th + 2 * MROWS * LDH);   // gamma
    float* SY = GM + H;                               // dy's row scales and
    float* RSY = SY + MROWS;                          //   their reciprocals (fixed for the kernel)
    float* RS = RSY + MROWS;                          // 1 / row scale of the tile mha_stage_acc staged last
    float* RMX = RS + MROWS;                          // [wave][row]: the waves' row maxima
    float* SCP = RMX + NWAVE * MROWS;                 // [wave][t][u][agent]: the waves' da partials
    const qs_mha_tower& t = tw.t[blockIdx.y];
    const qs_mha_train& tr = trs.t[blockIdx.y];
    const long ag0 = (long)blockIdx.x * MHA_AG;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, ag = lane & 31;
    constexpr size_t WBLK = (size_t)H * H * 2 * 2 / 16;
    constexpr float iSW = 1.f / X3_SW, iSX = 1.f / X3_SX, iSS = 1.f / (X3_SX * X3_SW);
    const size_t nblk = gridDim.x;
    auto cm_row = [&](int k) { return tr.colmax + ((size_t)k * nblk + blockIdx.x) * H; };
    auto wblk = [&](const void* w, int h) { return reinterpret_cast<const uint4*>(w) + h * WBLK; };

    for (int n = tid; n < H; n += NTHR) GM[n] = t.ln_g[n];
    {   // the saved tokens into X (zero rows past B; unconditional loads, agent 0 standing in)
        constexpr int NV = MROWS * (H / 4) / NTHR;
        float4 v[NV];
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int e = tid + u * NTHR, r = e / (H / 4), c4 = e - r * (H / 4);
            v[u] = ld4g(tr.x + mha_row(ag0, r, B) * H + 4 * c4);
        }
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int e = tid + u * NTHR, r = e / (H / 4), c4 = e - r * (H / 4);
            X.put4(r, 4 * c4, f4_scale(v[u], ag0 + (r & 31) < B ? X3_SX : 0.f));
        }
    }
    __syncthreads();

    // LayerNorm backward in the forward epilogue's row layout: wave w its rows [16 w, 16 w + 16), a row's H / 4 float4
    // on as many lanes; dy as fp32 rows into F, its row scales into SY / RSY
    {
        constexpr int LPR = H / 4, RPP = 64 / LPR;
        const int c4 = lane % LPR;
        const float4 gm = lds4(GM + 4 * c4);
        for (int r = 0; r < MROWS / NWAVE; r += RPP) {
            const int i = wave * (MROWS / NWAVE) + r + lane / LPR;
            const size_t row = mha_row(ag0, i, B);
            const float4 d = ld4g(tr.dout + row * H + 4 * c4), xn = ld4g(tr.xhat + row * H + 4 * c4);
            const float rsg = ag0 + (i & 31) < B ? tr.rsig[row] : 0.f;   // (0: a zero dy row past B)
            const float4 g = make_float4(d.x * gm.x, d.y * gm.y, d.z * gm.z, d.w * gm.w);
            float s1 = (g.x + g.y) + (g.z + g.w), s2 = (g.x * xn.x + g.y * xn.y) + (g.z * xn.z + g.w * xn.w);
#pragma unroll
            for (int m = LPR / 2; m >= 1; m >>= 1) {
                s1 += __shfl_xor(s1, m);
                s2 += __shfl_xor(s2, m);
            }
            const float m1 = s1 * (1.f / H), m2 = s2 * (1.f / H);
            const float4 dy = make_float4((g.x - m1 - xn.x * m2) * rsg, (g.y - m1 - xn.y * m2) * rsg,
                                          (g.z - m1 - xn.z * m2) * rsg, (g.w - m1 - xn.w * m2) * rsg);
            float mx = absmax4(dy);
#pragma unroll
            for (int m = LPR / 2; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
            if (c4 == 0) {
                const float s = row_scale(mx);
                SY[i] = s;
                RSY[i] = 1.f / s;
            }
            *reinterpret_cast<float4*>(F + i * LDF + 4 * c4) = dy;
        }
    }
    __syncthreads();
    // dy into the accumulator layout (both tokens of agent `ag` at the lane's columns), parked in HBM between its uses
    // like the running dX, which starts at dy: tr.dpre2 holds dy and tr.dpre1 holds dX until the last phase writes
    // those two gradients; a lane only ever reads back what it stored itself
    float* const dyp = tr.dpre2;
    float* const dXp = tr.dpre1;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int i = acc_i(rt, lane);
        if (ag0 + (i & 31) >= B) continue;
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n0 = acc_n0<H>(wave, c, g, lane);
                const float4 v = lds4(F + i * LDF + n0);
                st4g(dyp + mha_row(ag0, i, B) * H + n0, v);
                st4g(dXp + mha_row(ag0, i, B) * H + n0, v);
            }
    }
    const float itemp = 1.f / sqrtf((float)H);
    const float sy0 = SY[ag], sy1 = SY[MHA_AG + ag], ry0 = RSY[ag], ry1 = RSY[MHA_AG + ag];
    const size_t agc = ag0 + ag < B ? (size_t)(ag0 + ag) : 0;
    const size_t hrows = (size_t)B * 2 * H;   // one head's G_h / R_h

#pragma unroll 1
    for (int h = 0; h < MHA_HEADS; ++h) {
        f32x16 a[RT][CT], b[RT][CT];
        __syncthreads();   // every wave is past its reads of T (head 0: of F)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    T.put4(acc_i(rt, lane), acc_n0<H>(wave, c, g, lane),
                           f4_scale(mha_ld_own<H>(dyp, ag0, B, acc_i(rt, lane), acc_n0<H>(wave, c, g, lane)), rt ? sy1 : sy0));
        const float4 s4 = ld4g(tr.sm + (agc * MHA_HEADS + h) * 4);   // s[t][u] of the lane's agent
        const float s[2][2] = {{s4.x, s4.y}, {s4.z, s4.w}};
        __syncthreads();
        mfma_layer_x3<H>(T, wblk(tr.w_fctp, h), a, wave, lane);   // dctx (row-scaled)
        mfma_layer_x3<H>(X, wblk(t.w_vp, h), b, wave, lane);      // V
        // da[t][u] = dctx_t . v_u: this lane's columns, the other lane half's, then the four waves' after the barrier
        float p[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int tq = 0; tq < 2; ++tq)
#pragma unroll
                    for (int u = 0; u < 2; ++u) p[tq][u] = fmaf(a[tq][c][r], b[u][c][r], p[tq][u]);
#pragma unroll
        for (int tq = 0; tq < 2; ++tq)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                p[tq][u] += __shfl_xor(p[tq][u], 32);
                if (lane < 32) SCP[((wave * 2 + tq) * 2 + u) * MHA_AG + ag] = p[tq][u];
            }
        // G_h[u] = sum_t s[t][u] dy_t (lane-local), with its column maxima
        mha_store_rows<H, false>(tr.gmix + h * hrows, cm_row(4 + 2 * h), 0, ag0, B, wave, lane,
                                 [&](int u, int, int, int, int n0) {
                                     const float4 d0 = mha_ld_own<H>(dyp, ag0, B, ag, n0), d1 = mha_ld_own<H>(dyp, ag0, B, MHA_AG + ag, n0);
                                     return make_float4(s[0][u] * d0.x + s[1][u] * d1.x, s[0][u] * d0.y + s[1][u] * d1.y,
                                                        s[0][u] * d0.z + s[1][u] * d1.z, s[0][u] * d0.w + s[1][u] * d1.w);
                                 });
        // dv_u = sum_t s[t][u] dctx_t in place (dctx_t = a[t] / (dy's row scale, weight scale))
        {
            const float c0 = ry0 * iSW, c1 = ry1 * iSW;
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float d0 = a[0][c][r] * c0, d1 = a[1][c][r] * c1;
                    a[0][c][r] = s[0][0] * d0 + s[1][0] * d1;
                    a[1][c][r] = s[0][1] * d0 + s[1][1] * d1;
                }
        }
        __syncthreads();   // the partials are complete
        float ds[2][2];
#pragma unroll
        for (int tq = 0; tq < 2; ++tq) {
            float da[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float* pp = SCP + (tq * 2 + u) * MHA_AG + ag;
                da[u] = ((pp[0] + pp[4 * MHA_AG]) + (pp[8 * MHA_AG] + pp[12 * MHA_AG])) * ((tq ? ry1 : ry0) * iSW * iSS);
            }
            const float dot = s[tq][0] * da[0] + s[tq][1] * da[1];
#pragma unroll
            for (int u = 0; u < 2; ++u) ds[tq][u] = s[tq][u] * (da[u] - dot) * itemp;
        }
        mha_stage_acc<H>(T, a, RS, RMX, wave, lane);
        mfma_layer_x3<H>(T, wblk(tr.w_vtp, h), b, wave, lane);   // dv Wv_h
        mha_add_rows<H>(dXp, b, RS, ag0, B, wave, lane);
        mfma_layer_x3<H>(X, wblk(t.w_qp, h), a, wave, lane);     // Q, K
        mfma_layer_x3<H>(X, wblk(t.w_kp, h), b, wave, lane);
        // R_h[t] = sum_u ds[t][u] x_u
        mha_store_rows<H, false>(tr.rmix + h * hrows, cm_row(5 + 2 * h), 0, ag0, B, wave, lane,
                                 [&](int tq, int c, int g, int, int n0) {
                                     const float4 x0 = tile_get4(X, ag, n0), x1 = tile_get4(X, MHA_AG + ag, n0);
                                     const float w0 = ds[tq][0] * iSX, w1 = ds[tq][1] * iSX;
                                     return make_float4(w0 * x0.x + w1 * x1.x, w0 * x0.y + w1 * x1.y, w0 * x0.z + w1 * x1.z,
                                                        w0 * x0.w + w1 * x1.w);
                                 });
        // dq_t = sum_u ds[t][u] k_u over Q, dk_u = sum_t ds[t][u] q_t over K, in place
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float q0 = a[0][c][r] * iSS, q1 = a[1][c][r] * iSS, k0 = b[0][c][r] * iSS, k1 = b[1][c][r] * iSS;
                a[0][c][r] = ds[0][0] * k0 + ds[0][1] * k1;
                a[1][c][r] = ds[1][0] * k0 + ds[1][1] * k1;
                b[0][c][r] = ds[0][0] * q0 + ds[1][0] * q1;
                b[1][c][r] = ds[0][1] * q0 + ds[1][1] * q1;
            }
        mha_stage_acc<H>(T, a, RS, RMX, wave, lane);
        mfma_layer_x3<H>(T, wblk(tr.w_qtp, h), a, wave, lane);   // dq Wq_h (dq is staged: its registers take the product)
        mha_add_rows<H>(dXp, a, RS, ag0, B, wave, lane);
        mha_stage_acc<H>(T, b, RS, RMX, wave, lane);
        mfma_layer_x3<H>(T, wblk(tr.w_ktp, h), a, wave, lane);   // dk Wk_h
        mha_add_rows<H>(dXp, a, RS, ag0, B, wave, lane);
    }

    // the embedding layers: dpre2 = dX (1 - X^2) -> dx1 = dpre2 W_{n2|o2} -> dpre1 = dx1 (1 - x1^2)
    f32x16 dX[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = acc_i(rt, lane), n0 = acc_n0<H>(wave, c, g, lane);
                acc4_set(dX[rt][c], g, f4_dtanh(mha_ld_own<H>(dXp, ag0, B, i, n0), f4_scale(tile_get4(X, i, n0), iSX)));
            }
    mha_store_rows<H, true>(tr.dpre2, cm_row(0), nblk * H, ag0, B, wave, lane,
                            [&](int rt, int c, int g, int, int) { return acc4(dX[rt][c], g); });
    mha_stage_acc<H>(T, dX, RS, RMX, wave, lane);
    f32x16 a[RT][CT];
    {
        const uint4* const w2t[RT] = {reinterpret_cast<const uint4*>(tr.w_n2tp), reinterpret_cast<const uint4*>(tr.w_o2tp)};
        mfma_layer_x3_rt<H>(T, w2t, a, wave, lane);
    }
    mha_store_rows<H, true>(tr.dpre1, cm_row(2), nblk * H, ag0, B, wave, lane, [&](int rt, int c, int g, int i, int n0) {
        const float4 x1 = ld4g(tr.x1 + mha_row(ag0, i, B) * H + n0);
        return f4_dtanh(f4_scale(acc4(a[rt][c], g), RS[i] * iSW), x1);
    });
}

}  // namespace pol
}  // namespace qs
