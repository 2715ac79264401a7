// qs_policy_tail.h -- the rollout policy's tail as ONE kernel: from both towers' feed_forward outputs to (actions,
// values, log_prob).  Per tower (ActorCriticPolicyCustomSeparateWeights.forward, ActorCriticPolicyCustom.py:515-536,
// after the encoders):
//   chain   n_layers x (Linear + tanh): ModelCoreMLP's layers, then the MlpDecoder's; layer 0 is [R, 2R], the rest [R, R]
//   head    action_net [act_dim, Win] or value_net [1, Win]  (Win = R, or 2R with an empty chain)
//   actor   u = mean + exp(log_std) eps (or mean), a = tanh(u), log_prob = ppo.squashed_log_prob(mean, log_std, a)
//   critic  values = the head's output
//
// Work split: a 256-thread block owns 64 rows of one tower (grid: row tiles x towers).  The rows are loaded once,
// split into hi / lo f16 halves (qs_policy_x3.h TileX3) and stay in LDS until the head has read them; every chain
// layer is mfma_layer_x3 on that tile (wave w owns output columns [w R/4, (w + 1) R/4), the accumulators stay in
// registers) and its tanh epilogue writes the next layer's tile.  Nothing but the inputs, the weights and the three
// results touches HBM.
//
// LDS: the input tile X [64][2R + 8] (hi, lo).  Once every wave has read it (one barrier after layer 0), its bytes
// hold two [64][R + 8] tiles P0 / P1 that the remaining layers alternate between: a layer reads one and writes the
// other, so each layer costs one barrier (after its stores), not two.  Then the chain biases [n_layers][R] and the
// head's weights [n_out][Win] + bias, fp32.  R = 256: 135 168 + <= 16 416 bytes (one block per CU); R = 128: 69 632 +
// <= 8 224 bytes (two blocks per CU).
//
// Weights: each layer's packed operand (pack_mfma_weight_x3) streams from L2 behind mfma_layer_x3's two-step queue; the
// NEXT layer's first two steps (mfma_prefetch_x3) are issued before this layer's tanh epilogue, so they arrive while
// the epilogue and the barrier run.
//
// Head: fp32 VALU FMAs on x = (hi + lo) / 256 read back from the tile, not a padded MFMA.  n_out <= 8 would fill a
// quarter of a 32-column MFMA tile at best (1/32 for the critic), and the MFMA's f16 operands would put the split-f16
// range rule (|w| < 255.9) on action_net / value_net, whose weights nothing bounds; as FMAs the head takes plain fp32
// weights and costs 64 Win n_out / 256 <= 1024 FMAs per thread.  Four adjacent lanes share a row (each a quarter of
// its 8-column chunks) and add their partial sums with two shuffles; lane 0 of the four runs the row's epilogue.
//
// log_prob is evaluated on the fp32 action that is stored (the update recomputes it from the stored action): clamp to
// +-(1 - 2^-23), atanh as (log1p(y) - log1p(-y)) / 2, the Gaussian term, minus sum log(1 - a^2 + 1e-6) with 1 - a^2
// as one fma (one rounding of the exact value: the product a a alone would lose 1 / (1 - a^2) ulps).
#pragma once
#include "qs_policy_x3.h"

namespace qs {
namespace pol {

struct TailTowers {
    qs_tail_tower t[QS_ATTN_MAX_TOWERS];
};

template <int R>
struct TailGeo {
    static constexpr int W0 = 2 * R;
    static constexpr int LD0 = GeoX3<W0>::LDH, LDR = GeoX3<R>::LDH;
    static constexpr int X_HALVES = 2 * MROWS * LD0;      // the input tile, hi + lo
    static constexpr int P_HALVES = 2 * MROWS * LDR;      // one chain tile, hi + lo
    static constexpr int TILE_HALVES = X_HALVES > 2 * P_HALVES ? X_HALVES : 2 * P_HALVES;
};
template <int R>
constexpr size_t tail_lds_bytes(int n_layers, int n_out) {
    return (size_t)TailGeo<R>::TILE_HALVES * 2 +
           (size_t)(n_layers * R + n_out * (n_layers ? R : 2 * R) + QS_TAIL_MAX_OUT) * 4;
}

// the block's rows of X [B, 2R] (fp32, HBM) into the split tile, scaled by X3_SX; zero rows past B.  Eight float4 per
// thread in flight at a time (unconditional loads: row 0 stands in past B, see qs_policy.h acc_from_P)
template <int R>
__device__ __forceinline__ void tail_load_rows(const TileX3& X, const float* __restrict__ src, long row0, long B, int tid) {
    constexpr int W4 = 2 * R / 4, NV = MROWS * W4 / NTHR, CH = 8;
    static_assert(NV % CH == 0, "whole chunks");
    for (int u0 = 0; u0 < NV; u0 += CH) {
        float4 v[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int e = tid + (u0 + u) * NTHR, r = e / W4, c4 = e - r * W4;
            const bool ok = row0 + r < B;
            v[u] = f4_scale(reinterpret_cast<const float4*>(src + (ok ? row0 + r : 0) * (long)(2 * R))[c4], ok ? X3_SX : 0.f);
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int e = tid + (u0 + u) * NTHR, r = e / W4, c4 = e - r * W4;
            X.put4(r, 4 * c4, v[u]);
        }
    }
}

// sum_k x[r][k] w[o][k] for this lane's quarter of row r's 8-column chunks, x = hi + lo (scaled by X3_SX)
__device__ __forceinline__ void tail_head_partials(const TileX3& T, const float* HW, int Win, int n_out, int r, int q,
                                                   float (&s)[QS_TAIL_MAX_OUT]) {
#pragma unroll
    for (int o = 0; o < QS_TAIL_MAX_OUT; ++o) s[o] = 0.f;
    for (int k0 = 8 * q; k0 < Win; k0 += 32) {
        const f16x8 h = *reinterpret_cast<const f16x8*>(T.h + r * T.ld + k0);
        const f16x8 l = *reinterpret_cast<const f16x8*>(T.l + r * T.ld + k0);
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = (float)h[j] + (float)l[j];
#pragma unroll
        for (int o = 0; o < QS_TAIL_MAX_OUT; ++o) {
            if (o < n_out) {   // (uniform)
                const float4 w0 = lds4(HW + o * Win + k0), w1 = lds4(HW + o * Win + k0 + 4);
                s[o] = fmaf(x[0], w0.x, s[o]); s[o] = fmaf(x[1], w0.y, s[o]);
                s[o] = fmaf(x[2], w0.z, s[o]); s[o] = fmaf(x[3], w0.w, s[o]);
                s[o] = fmaf(x[4], w1.x, s[o]); s[o] = fmaf(x[5], w1.y, s[o]);
                s[o] = fmaf(x[6], w1.z, s[o]); s[o] = fmaf(x[7], w1.w, s[o]);
            }
        }
    }
#pragma unroll
    for (int o = 0; o < QS_TAIL_MAX_OUT; ++o) {
        s[o] += __shfl_xor(s[o], 1);
        s[o] += __shfl_xor(s[o], 2);
    }
}

// one row's results from its head outputs m[o] (already descaled, bias added)
__device__ __forceinline__ void tail_row_epilogue(const qs_tail_tower& t, long row, const float (&m)[QS_TAIL_MAX_OUT]) {
    const int n_out = t.n_out;
    float* out = t.out + row * n_out;
    if (!t.log_std) {   // critic: the head's outputs
#pragma unroll
        for (int o = 0; o < QS_TAIL_MAX_OUT; ++o)
            if (o < n_out) out[o] = m[o];
        return;
    }
    const bool sample = !t.deterministic && t.eps;
    const float one = 1.f - 1.1920929e-07f;   // 1 - fp32 eps (TanhBijector.inverse's clamp)
    float gauss = 0.f, jac = 0.f;
#pragma unroll
    for (int o = 0; o < QS_TAIL_MAX_OUT; ++o) {
        if (o < n_out) {
            const float ls = t.log_std[o];
            const float u = sample ? fmaf(expf(ls), t.eps[row * n_out + o], m[o]) : m[o];
            const float a = tanhf(u);
            out[o] = a;
            const float y = fminf(fmaxf(a, -one), one);
            const float g = 0.5f * (log1pf(y) - log1pf(-y));
            const float z = (g - m[o]) * expf(-ls);
            gauss += -0.5f * z * z - ls - 0.91893853320467274f;   // log sqrt(2 pi)
            jac += logf(fmaf(-a, a, 1.f) + 1e-6f);
        }
    }
    t.log_prob[row] = gauss - jac;
}

template <int R>
__global__ __launch_bounds__(NTHR, R == 128 ? 2 : 1) void policy_tail_x3_kernel(long B, int n_layers, TailTowers tw) {
    using G = TailGeo<R>;
    constexpr int CT = Geo<R>::CT;
    constexpr float iSS = 1.f / (X3_SX * X3_SW);
    extern __shared__ float4 smem4[];
    _Float16* th = reinterpret_cast<_Float16*>(smem4);
    const TileX3 X{th, th + MROWS * G::LD0, G::LD0};
    const TileX3 P0{th, th + MROWS * G::LDR, G::LDR};
    const qs_tail_tower& t = tw.t[blockIdx.y];
    const int n_out = t.n_out, Win = n_layers ? R : 2 * R;
    float* BI = reinterpret_cast<float*>(th + G::TILE_HALVES);   // chain biases [n_layers][R]
    float* HW = BI + n_layers * R;                               // head weights [n_out][Win], then its bias
    float* HB = HW + n_out * Win;
    const long row0 = (long)blockIdx.x * MROWS;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

    tail_load_rows<R>(X, t.x, row0, B, tid);
    for (int l = 0; l < n_layers; ++l)
        for (int n = tid; n < R; n += NTHR) BI[l * R + n] = t.b_chain[l][n];
    for (int e = tid; e < n_out * Win; e += NTHR) HW[e] = t.w_head[e];
    if (tid < n_out) HB[tid] = t.b_head[tid];
    __syncthreads();

    TileX3 cur = X;   // the tile the next stage reads
    if (n_layers > 0) {
        f32x16 acc[RT][CT];
        WQueue<R> q;
        mfma_layer_x3<R, 2 * R>(X, reinterpret_cast<const uint4*>(t.w_chain[0]), acc, wave, lane);
        if (n_layers > 1) q = mfma_prefetch_x3<R>(reinterpret_cast<const uint4*>(t.w_chain[1]), wave, lane);
        __syncthreads();   // every wave has read X: P0 lies over it
        store_tanh_x3<R>(P0, acc, iSS, wave, lane, [&](int, int n0) { return lds4(BI + n0); });
        __syncthreads();
        cur = P0;
        for (int l = 1; l < n_layers; ++l) {   // reads one of P0 / P1, writes the other: one barrier per layer
            _Float16* pb = th + (l & 1) * G::P_HALVES;
            const TileX3 dst{pb, pb + MROWS * G::LDR, G::LDR};
            mfma_layer_x3<R, R>(cur, reinterpret_cast<const uint4*>(t.w_chain[l]), acc, wave, lane, q);
            if (l + 1 < n_layers) q = mfma_prefetch_x3<R>(reinterpret_cast<const uint4*>(t.w_chain[l + 1]), wave, lane);
            const float* bl = BI + l * R;
            store_tanh_x3<R>(dst, acc, iSS, wave, lane, [&](int, int n0) { return lds4(bl + n0); });
            __syncthreads();
            cur = dst;
        }
    }

    const int r = tid >> 2, qd = tid & 3;
    float s[QS_TAIL_MAX_OUT];
    tail_head_partials(cur, HW, Win, n_out, r, qd, s);
    if (qd == 0 && row0 + r < B) {
#pragma unroll
        for (int o = 0; o < QS_TAIL_MAX_OUT; ++o) s[o] = o < n_out ? fmaf(s[o], 1.f / X3_SX, HB[o]) : 0.f;
        tail_row_epilogue(t, row0 + r, s);
    }
}

}  // namespace pol
}  // namespace qs
