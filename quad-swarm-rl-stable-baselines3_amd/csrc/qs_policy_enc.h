// qs_policy_enc.h -- fused no-grad forward of QuadMultiEncoder for the neighbour encoders that are plain MLPs (mlp,
// mean_embed, no_encoder), on the split-f16 matrix cores (precision x3 only; qs_policy_x3.h's tile, layer and scales).
//
// QuadMultiEncoder (swarm_rl/models/quad_multi_model.py:250-353) per agent, every layer Linear + tanh:
//   s = self_encoder(obs[:so])                                          2 layers
//   n = neighbor_mlp(obs[so : so + K nd])                               QuadNeighborhoodEncoderMlp, 3 layers       (mlp)
//     = mean_k embedding_mlp(obs[so + k nd : so + (k + 1) nd])          QuadNeighborhoodEncoderDeepsets, 2 layers  (mean)
//   o = obstacle_encoder(obs[so + K nd : so + K nd + od])               2 layers, when od > 0
//   out = tanh([s | n | o] W_ff^T + b_ff)                               feed_forward, [B, 2H]
// i.e. from the raw observations to the rows qs_policy_tail_x3 reads: one launch for both towers, each tower's
// weights read once, no intermediate tensor, no concatenation.
//
// Row split: a block owns 64 agents as the 64 rows of the tile, one agent per row in every branch.  The deep-sets mean
// therefore never crosses a lane: in the accumulator layout (qs_policy.h acc_i / acc_n0) lane l holds the same agents'
// columns for every neighbour k, so sum_k e_k is a register accumulation over the loop "for k: the 64 agents'
// neighbour k" (the rows are agents, not (agent, neighbour) pairs as in attn_embed_x3_kernel).
//
// Branches in the order self, neighbour, obstacle; each leaves a part tile P [64][H] of tanh outputs in LDS, and the
// feed_forward accumulates accff[z] += P W_ff[zH:(z+1)H, pH:(p+1)H]^T for both output halves z right after part p:
// only one part is resident, the concatenation is never formed.  Layer 0 of a branch contracts over its own zero-padded
// width (self 32, mlp block 64, one neighbour 16, obstacles 16) from a gathered tile at X3_SIN.
//
// LDS: two split-f16 tiles [64][H + 8] (hi, lo) that the layers alternate between (a layer reads one and writes the
// other: one barrier per layer); a branch's gathered layer-0 input lies in the one that holds no part.  Then the bias
// table, 9 H floats.  H = 256: 135 168 + 9 216 B, one block per CU; H = 128: 69 632 + 4 608 B, two blocks per CU.
// Registers at H = 256: accff 2 x 64, the working accumulator 64, the mean's sum 64 (NBR mean only), plus the weight
// queue and the A operands of mfma_layer_x3 -- no scratch (DESIGN.md §4 has the resource-usage lines).
//
// At the end of the file: enc_join_x3_kernel, the same segment for the two attention families, whose neighbour part(s)
// come from their own kernels' output rows instead of a branch here (qs_encoder_join_x3).
#pragma once
#include "qs_policy_x3.h"

namespace qs {
namespace pol {

constexpr int ENC_SW = 32;    // self layer 0's contraction width (self_dim <= 32)
constexpr int ENC_NBW = 64;   // the mlp neighbour block's (K nd <= 64)
constexpr int ENC_NDW = 16;   // one neighbour's (mean: nd <= 16)
constexpr int ENC_OBW = 16;   // the obstacle values' (od <= 16)

struct EncTowers {
    qs_enc_tower t[QS_ATTN_MAX_TOWERS];
};

template <int H>
constexpr size_t enc_lds_bytes() {
    return (size_t)(4 * MROWS * GeoX3<H>::LDH) * 2 + (size_t)(9 * H) * 4;
}

__device__ __forceinline__ TileX3 enc_tile(_Float16* base, int ld) { return TileX3{base, base + MROWS * ld, ld}; }

// A branch's layer-0 input tile [64][W] at X3_SIN: row r = agent row0 + r, columns [0, n) = obs[agent][col0 .. col0 + n),
// the rest zero.  Loads unconditional and back to back (qs_policy_mha.h mha_gather0): a column past the data reads the
// agent's word 0 and a row past B reads obs[0], both zeroed by a product.
template <int W>
__device__ __forceinline__ void enc_gather0(const TileX3& X0, const float* __restrict__ obs, int stride, int col0, int n,
                                            int B, long row0, int tid) {
    constexpr int NV = MROWS * W / NTHR;
    float v[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int e = tid + u * NTHR, r = e / W, c = e - r * W;
        const bool okr = row0 + r < B, ok = okr && c < n;
        v[u] = obs[(okr ? (size_t)(row0 + r) * stride : 0) + (ok ? col0 + c : 0)] * (ok ? X3_SIN : 0.f);
    }
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int e = tid + u * NTHR;
        X0.put(e / W, e % W, v[u]);
    }
}

// layer 0: the gathered tile (in src's bytes) -> tanh rows in dst; then every wave may read dst and overwrite src
template <int H, int W>
__device__ __forceinline__ void enc_layer0(_Float16* src, _Float16* dst, const void* wp, const float* bias,
                                           f32x16 (&acc)[RT][Geo<H>::CT], int wave, int lane) {
    mfma_layer_x3<H, W, true, false>(enc_tile(src, GeoX3<W>::LDH), reinterpret_cast<const uint4*>(wp), acc, wave, lane);
    store_tanh_x3<H>(enc_tile(dst, GeoX3<H>::LDH), acc, 1.f / (X3_SIN * X3_SW), wave, lane,
                     [&](int, int n0) { return lds4(bias + n0); });
    __syncthreads();
}
// an H x H layer: tanh rows in src -> tanh rows in dst
template <int H>
__device__ __forceinline__ void enc_layer(_Float16* src, _Float16* dst, const void* wp, const float* bias,
                                          f32x16 (&acc)[RT][Geo<H>::CT], int wave, int lane) {
    mfma_layer_x3<H>(enc_tile(src, GeoX3<H>::LDH), reinterpret_cast<const uint4*>(wp), acc, wave, lane);
    store_tanh_x3<H>(enc_tile(dst, GeoX3<H>::LDH), acc, 1.f / (X3_SX * X3_SW), wave, lane,
                     [&](int, int n0) { return lds4(bias + n0); });
    __syncthreads();
}
// the feed_forward's share of part p (the tile in part's bytes): accff[z] (+)= P W_ff[zH .., pH ..]^T
template <int H, bool ZERO>
__device__ __forceinline__ void enc_ff(_Float16* part, const void* wffp, int NP, int p,
                                       f32x16 (&accff)[2][RT][Geo<H>::CT], int wave, int lane) {
    constexpr size_t WBLK = (size_t)H * H * 2 * 2 / 16;   // uint4 per packed H x H block
    const TileX3 P = enc_tile(part, GeoX3<H>::LDH);
#pragma unroll
    for (int z = 0; z < 2; ++z)
        mfma_layer_x3<H, H, ZERO>(P, reinterpret_cast<const uint4*>(wffp) + (size_t)(z * NP + p) * WBLK, accff[z], wave, lane);
}

// raw observations -> the feed_forward output out [B, 2H] of one tower (blockIdx.y), 64 agents per block.
// NBR: qs_enc_nbr_kind.  K, nd: the neighbour block's shape (it is skipped over to the obstacle values when NBR is none).
template <int H, int NBR>
__global__ __launch_bounds__(NTHR, H == 256 ? 1 : 2) void enc_mlp_x3_kernel(const float* __restrict__ obs, int stride,
                                                                           int so, int K, int nd, int od, int B,
                                                                           EncTowers tw) {
    constexpr int LDH = GeoX3<H>::LDH, CT = Geo<H>::CT, TH = 2 * MROWS * LDH;
    static_assert(GeoX3<ENC_NBW>::LDH <= LDH, "every layer-0 input tile fits a tile's bytes");
    constexpr float iSS = 1.f / (X3_SX * X3_SW);
    extern __shared__ float4 smem4[];
    _Float16* th = reinterpret_cast<_Float16*>(smem4);
    _Float16 *ta = th, *tb = th + TH;   // ta: the tile that holds no part (the next gather's and layer's target)
    float* BI = reinterpret_cast<float*>(th + 2 * TH);   // b_s1, b_s2, b_n1, b_n2, b_n3, b_o1, b_o2, b_ff [2H]
    const qs_enc_tower& t = tw.t[blockIdx.y];
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
    // self: the part ends in the gather's own tile
    enc_gather0<ENC_SW>(enc_tile(ta, GeoX3<ENC_SW>::LDH), obs, stride, 0, so, B, row0, tid);
    __syncthreads();
    enc_layer0<H, ENC_SW>(ta, tb, t.w_s1p, BI, acc, wave, lane);
    enc_layer<H>(tb, ta, t.w_s2p, BI + H, acc, wave, lane);
    enc_ff<H, true>(ta, t.w_ffp, NP, p++, accff, wave, lane);
    swap();

    if constexpr (NBR == QS_ENC_NBR_MLP) {   // three layers: the part ends in the other tile
        enc_gather0<ENC_NBW>(enc_tile(ta, GeoX3<ENC_NBW>::LDH), obs, stride, so, K * nd, B, row0, tid);
        __syncthreads();   // (and every wave is past the previous part's feed_forward reads)
        enc_layer0<H, ENC_NBW>(ta, tb, t.w_n1p, BI + 2 * H, acc, wave, lane);
        enc_layer<H>(tb, ta, t.w_n2p, BI + 3 * H, acc, wave, lane);
        enc_layer<H>(ta, tb, t.w_n3p, BI + 4 * H, acc, wave, lane);
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
        for (int k = 0; k < K; ++k) {   // the 64 agents' neighbour k
            enc_gather0<ENC_NDW>(enc_tile(ta, GeoX3<ENC_NDW>::LDH), obs, stride, so + k * nd, nd, B, row0, tid);
            __syncthreads();   // (and every wave is past its reads of tb: the feed_forward's, or neighbour k - 1's layer)
            enc_layer0<H, ENC_NDW>(ta, tb, t.w_n1p, BI + 2 * H, acc, wave, lane);
            mfma_layer_x3<H>(enc_tile(tb, LDH), reinterpret_cast<const uint4*>(t.w_n2p), acc, wave, lane);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)   // e_k = tanh(. + b_n2) added in registers: lane l, the same agents for every k
#pragma unroll
                for (int c = 0; c < CT; ++c)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        acc4_set(sum[rt][c], g,
                                 f4_add(acc4(sum[rt][c], g),
                                        tanh_bias4(acc[rt][c], g, iSS, lds4(BI + 3 * H + acc_n0<H>(wave, c, g, lane)))));
        }
        const TileX3 P = enc_tile(ta, LDH);   // (layer 0's input tile: last read before its barrier)
        // the mean as sum (1 / K), rounded to fp32, THEN the tile's scale: put4's hi half and the residual its lo half
        // is taken from must see one value.  With a single factor 256 / K (no power of two) the compiler rounds hi from
        // the exact product and the residual from the fp32 one, which differ by an f16 ulp next to a tie (2^-13 of the
        // elements, measured: 1.2e-4 absolute on one latent in 16 384).
        const float ik = 1.f / (float)K;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    P.put4(acc_i(rt, lane), acc_n0<H>(wave, c, g, lane),
                           f4_scale(f4_scale(acc4(sum[rt][c], g), ik), X3_SX));   // (exact: 2^8)
        __syncthreads();
        enc_ff<H, false>(ta, t.w_ffp, NP, p++, accff, wave, lane);
        swap();
    }
    if (od > 0) {   // (uniform) the offset counts the neighbour block whether or not an encoder read it
        enc_gather0<ENC_OBW>(enc_tile(ta, GeoX3<ENC_OBW>::LDH), obs, stride, so + K * nd, od, B, row0, tid);
        __syncthreads();
        enc_layer0<H, ENC_OBW>(ta, tb, t.w_o1p, BI + 5 * H, acc, wave, lane);
        enc_layer<H>(tb, ta, t.w_o2p, BI + 6 * H, acc, wave, lane);
        enc_ff<H, false>(ta, t.w_ffp, NP, p++, accff, wave, lane);
    }

    // out[agent][zH + n] = tanh(accff[z] + b_ff), 16-byte stores, rows < B
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
// The attention families' join (qs_encoder_join_x3): what follows their neighbour kernels up to the rows the tail reads.
//   QuadMultiEncoder, neighbor_encoder_type "attention":  out = tanh([s | pooled | o] W_ff^T + b_ff)        NQ = 1
//   QuadMultiHeadAttentionEncoder:                        out = tanh([s | token 0 | token 1] W_ff^T + b_ff)  NQ = 2
// s and o are the self and obstacle branches of enc_mlp_x3_kernel (the same helpers, tiles and choreography); a
// neighbour part is not computed here but staged: rows nbr[agent][qH .. (q + 1)H) (fp32, written by attn_pool_x3_kernel /
// mha_encoder_x3_kernel) go through put4 at X3_SX into the tile that holds no part, then enc_ff.  Every part is at X3_SX,
// so all of them accumulate into one accff at one scale; the tokens are LayerNorm outputs, bounded by the caller
// (policy_fused: sqrt(H) max |ln_g| + max |ln_b| inside the f16 range at X3_SX).
//
// The row loads are the only HBM reads of activations on the block's path.  They are issued first, all NQ parts, 16 B per
// lane and fully coalesced (a row is H / 4 consecutive lanes), and held in registers (NQ x 16 float4 per thread at H =
// 256, NQ x 8 at 128) across the self branch: the memory counter retires in order, so the self gather's wait covers them
// too and one HBM latency is paid per block instead of one per part.  The scheduling fences of the self branch's layers
// keep the loads where they are written.  Registers at H = 256: accff 128 + acc 64 + the held rows 64 / 128 + the weight
// queue, inside the 512 of one wave per SIMD -- no scratch.
// LDS: the two alternating tiles and a 6 H float bias table: 135 168 + 6 144 B at H = 256 (one block per CU), 69 632 +
// 3 072 B at H = 128 (two).
struct JoinTowers {
    qs_join_tower t[QS_ATTN_MAX_TOWERS];
};

template <int H>
constexpr size_t join_lds_bytes() {
    return (size_t)(4 * MROWS * GeoX3<H>::LDH) * 2 + (size_t)(6 * H) * 4;
}

template <int H>
struct JoinRows {
    static constexpr int NV = MROWS * (H / 4) / NTHR;
    float4 v[NV];
    // part q of the block's 64 agents; unconditional loads (row 0 stands in past B, zeroed by put's scale)
    __device__ __forceinline__ void load(const float* __restrict__ nbr, int ldn, int q, int B, long row0, int tid) {
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int e = tid + u * NTHR, r = e / (H / 4), c4 = e - r * (H / 4);
            v[u] = *reinterpret_cast<const float4*>(nbr + (row0 + r < B ? (size_t)(row0 + r) * ldn : 0) + q * H + 4 * c4);
        }
    }
    __device__ __forceinline__ void put(const TileX3& P, int B, long row0, int tid) const {
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int e = tid + u * NTHR, r = e / (H / 4), c4 = e - r * (H / 4);
            P.put4(r, 4 * c4, f4_scale(v[u], row0 + r < B ? X3_SX : 0.f));   // (exact: 2^8)
        }
    }
};

// raw observations and the neighbour kernels' rows -> the feed_forward output out [B, 2H] of one tower (blockIdx.y),
// 64 agents per block.  NQ: neighbour parts (1 pooled row, 2 tokens); oo, od: the obstacle values' column and count.
template <int H, int NQ>
__global__ __launch_bounds__(NTHR, H == 256 ? 1 : 2) void enc_join_x3_kernel(const float* __restrict__ obs, int stride,
                                                                            int so, int oo, int od, int B, JoinTowers tw) {
    constexpr int LDH = GeoX3<H>::LDH, CT = Geo<H>::CT, TH = 2 * MROWS * LDH;
    constexpr float iSS = 1.f / (X3_SX * X3_SW);
    extern __shared__ float4 smem4[];
    _Float16* th = reinterpret_cast<_Float16*>(smem4);
    _Float16 *ta = th, *tb = th + TH;   // ta: the tile that holds no part (the next staging's, gather's and layer's target)
    float* BI = reinterpret_cast<float*>(th + 2 * TH);   // b_s1, b_s2, b_o1, b_o2, b_ff [2H]
    const qs_join_tower& t = tw.t[blockIdx.y];
    const long row0 = (long)blockIdx.x * MROWS;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int NP = 1 + NQ + (od > 0 ? 1 : 0);

    JoinRows<H> rows[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) rows[q].load(t.nbr, NQ * H, q, B, row0, tid);

    for (int n = tid; n < H; n += NTHR) {
        BI[n] = t.b_s1[n];
        BI[H + n] = t.b_s2[n];
        if (od > 0) {
            BI[2 * H + n] = t.b_o1[n];
            BI[3 * H + n] = t.b_o2[n];
        }
        BI[4 * H + n] = t.b_ff[n];
        BI[5 * H + n] = t.b_ff[H + n];
    }
    auto swap = [&]() {
        _Float16* x = ta;
        ta = tb;
        tb = x;
    };

    f32x16 acc[RT][CT], accff[2][RT][CT];
    // self: the part ends in the gather's own tile
    enc_gather0<ENC_SW>(enc_tile(ta, GeoX3<ENC_SW>::LDH), obs, stride, 0, so, B, row0, tid);
    __syncthreads();
    enc_layer0<H, ENC_SW>(ta, tb, t.w_s1p, BI, acc, wave, lane);
    enc_layer<H>(tb, ta, t.w_s2p, BI + H, acc, wave, lane);
    enc_ff<H, true>(ta, t.w_ffp, NP, 0, accff, wave, lane);
    swap();

#pragma unroll
    for (int q = 0; q < NQ; ++q) {   // ta was last read before a barrier every wave has passed (enc_mlp_x3_kernel's order)
        rows[q].put(enc_tile(ta, LDH), B, row0, tid);
        __syncthreads();
        enc_ff<H, false>(ta, t.w_ffp, NP, 1 + q, accff, wave, lane);
        swap();
    }
    if (od > 0) {   // (uniform)
        enc_gather0<ENC_OBW>(enc_tile(ta, GeoX3<ENC_OBW>::LDH), obs, stride, oo, od, B, row0, tid);
        __syncthreads();
        enc_layer0<H, ENC_OBW>(ta, tb, t.w_o1p, BI + 2 * H, acc, wave, lane);
        enc_layer<H>(tb, ta, t.w_o2p, BI + 3 * H, acc, wave, lane);
        enc_ff<H, false>(ta, t.w_ffp, NP, 1 + NQ, accff, wave, lane);
    }

    // out[agent][zH + n] = tanh(accff[z] + b_ff), 16-byte stores, rows < B
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
                         tanh_bias4(accff[z][rt][c], g, iSS, lds4(BI + (4 + z) * H + n0)));
                }
        }
}

}  // namespace pol
}  // namespace qs
