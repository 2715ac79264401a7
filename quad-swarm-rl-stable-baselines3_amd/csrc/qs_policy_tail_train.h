// qs_policy_tail_train.h -- the PPO update's policy tail on the split-f16 matrix cores: what qs_policy_tail.h is to the
// rollout, for PPOTrainer.train.  Per tower, from the feed_forward output X [B, 2R] and (actor) the stored actions:
//   forward   policy_tail_train_x3_kernel: the rollout kernel's phase sequence and arithmetic (64-row tile per block,
//             split tile in LDS, mfma_layer_x3 per chain layer, the fp32 FMA head), written out a second time (a body
//             shared with the rollout kernel would carry the save sink's address arithmetic into the rollout instance;
//             DESIGN.md §4 on the encoders).  It differs in three places: every chain layer's fp32 tanh output y[l] is
//             also stored (store_tanh_x3's sink; rows that exist only), the actor reads the stored actions instead of
//             noise and writes mean and log_prob of THOSE actions (tail_row_epilogue's expressions), the critic values.
//   backward  policy_tail_bwd_x3_kernel, from dvalues [B, 1] / dlogp [B] and the saves:
//               head   dout[r][o] (critic: dvalues; actor: dlogp z_o / sigma_o, z_o = (atanh(a_o) - mean_o) / sigma_o,
//                      and dlogp (z_o^2 - 1) for log_std), dy_L = dout W_head (fp32 FMAs), the head's dW / db parts
//               chain  l = L-1 .. 0: dpre_l = dy_l (1 - y_l^2) -> HBM (the weight gradient's G operand) and, each row at
//                      its own power-of-two scale, into one split gradient tile; dy_{l-1} = dpre_l W_l on
//                      mfma_layer_x3 with W_l^T packed like any weight; layer 0 ([R, 2R]) as two R x R blocks of
//                      W_0^T on the same staged tile -> the two halves of dlat [B, 2R]
//             The weight gradients dpre_l^T y_{l-1} are qs_dw_x3_ld's (quadswarm_amd/tail_train.py).
//
// Backward work split: a block per tower WALKS 64-row tiles with stride gridDim.x (the host sizes the grid from the CU
// count, capped by the number of tiles), so that what a block reduces over rows -- the head's weight gradient
// [n_out][Win + 1], the log_std sums, the column maxima of every dpre_l -- is kept across its tiles (registers: a
// thread owns head columns k = tid, tid + 256 for all outputs; LDS: the maxima) and written once per block: the
// partials the host sums do not grow with B (per 64-row tile, the head gradient alone would be 36 MB at 262 144 rows).
// Within a tile the gradient lives in the accumulator registers from the head's dy to dlat: each layer's y_l is loaded
// at the lane's accumulator positions (issued before the previous layer's MFMAs), the tanh derivative, the dpre store,
// the column maxima and the row-scaled staging happen in one pass over the registers (qs_policy_train.h
// stage_acc_scaled), and the product's scale comes off in the next pass.
//
// LDS: one [64][R + 8] hi / lo gradient tile, the row scales RS [64] and their reduction scratch [4][64], dout and the
// log_std terms [64][8] each, the head weights [n_out][Win], the column maxima [n_layers][R].  R = 256: 67 584 + <=
// 21 760 bytes (one block per CU); R = 128: 34 816 + <= 13 568 bytes (two blocks per CU by the launch bound).
//
// Zero gradients are the normal case (PPO's clip zeroes dlogp on clipped rows): a zero row takes scale 1 (row_scale)
// and contributes exact zeros; a non-finite value marks its column maximum +inf, as in the encoders' backward.
#pragma once
#include "qs_policy_tail.h"
#include "qs_policy_train.h"

namespace qs {
namespace pol {

struct TailTrains {
    qs_tail_train t[QS_ATTN_MAX_TOWERS];
};

// ------------------------------------------------------------------------------------------------------------------
// forward with saves
// ------------------------------------------------------------------------------------------------------------------
// one row's results from its head outputs m[o]: tail_row_epilogue with the action read, not drawn
__device__ __forceinline__ void tail_train_row_epilogue(const qs_tail_tower& t, const qs_tail_train& tr, long row,
                                                        const float (&m)[QS_TAIL_MAX_OUT]) {
    const int n_out = t.n_out;
    if (!t.log_std) {   // critic: the head's outputs
        float* out = t.out + row * n_out;
#pragma unroll
        for (int o = 0; o < QS_TAIL_MAX_OUT; ++o)
            if (o < n_out) out[o] = m[o];
        return;
    }
    const float one = 1.f - 1.1920929e-07f;
    float gauss = 0.f, jac = 0.f;
#pragma unroll
    for (int o = 0; o < QS_TAIL_MAX_OUT; ++o) {
        if (o < n_out) {
            const float ls = t.log_std[o];
            const float a = tr.actions[row * n_out + o];
            tr.mean[row * n_out + o] = m[o];
            const float y = fminf(fmaxf(a, -one), one);
            const float g = 0.5f * (log1pf(y) - log1pf(-y));
            const float z = (g - m[o]) * expf(-ls);
            gauss += -0.5f * z * z - ls - 0.91893853320467274f;
            jac += logf(fmaf(-a, a, 1.f) + 1e-6f);
        }
    }
    t.log_prob[row] = gauss - jac;
}

template <int R>
__global__ __launch_bounds__(NTHR, R == 128 ? 2 : 1) void policy_tail_train_x3_kernel(long B, int n_layers, TailTowers tw,
                                                                                      TailTrains trs) {
    using G = TailGeo<R>;
    constexpr int CT = Geo<R>::CT;
    constexpr float iSS = 1.f / (X3_SX * X3_SW);
    extern __shared__ float4 smem4[];
    _Float16* th = reinterpret_cast<_Float16*>(smem4);
    const TileX3 X{th, th + MROWS * G::LD0, G::LD0};
    const TileX3 P0{th, th + MROWS * G::LDR, G::LDR};
    const qs_tail_tower& t = tw.t[blockIdx.y];
    const qs_tail_train& tr = trs.t[blockIdx.y];
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

    TileX3 cur = X;
    if (n_layers > 0) {
        f32x16 acc[RT][CT];
        WQueue<R> q;
        mfma_layer_x3<R, 2 * R>(X, reinterpret_cast<const uint4*>(t.w_chain[0]), acc, wave, lane);
        if (n_layers > 1) q = mfma_prefetch_x3<R>(reinterpret_cast<const uint4*>(t.w_chain[1]), wave, lane);
        __syncthreads();   // every wave has read X: P0 lies over it
        float* y0 = tr.y[0];
        store_tanh_x3<R>(P0, acc, iSS, wave, lane, [&](int, int n0) { return lds4(BI + n0); },
                         [&](int i, int n0, float4 y) {
                             if (row0 + i < B) st4g(y0 + (row0 + i) * R + n0, y);
                         });
        __syncthreads();
        cur = P0;
        for (int l = 1; l < n_layers; ++l) {   // the next layer's first weights are fetched ahead of y[l]'s stores
            _Float16* pb = th + (l & 1) * G::P_HALVES;
            const TileX3 dst{pb, pb + MROWS * G::LDR, G::LDR};
            mfma_layer_x3<R, R>(cur, reinterpret_cast<const uint4*>(t.w_chain[l]), acc, wave, lane, q);
            if (l + 1 < n_layers) q = mfma_prefetch_x3<R>(reinterpret_cast<const uint4*>(t.w_chain[l + 1]), wave, lane);
            const float* bl = BI + l * R;
            float* yl = tr.y[l];
            store_tanh_x3<R>(dst, acc, iSS, wave, lane, [&](int, int n0) { return lds4(bl + n0); },
                             [&](int i, int n0, float4 y) {
                                 if (row0 + i < B) st4g(yl + (row0 + i) * R + n0, y);
                             });
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
        tail_train_row_epilogue(t, tr, row0 + r, s);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------
template <int R>
constexpr size_t tail_bwd_lds_bytes(int n_layers, int n_out) {
    return (size_t)(2 * MROWS * GeoX3<R>::LDH) * 2 +
           (size_t)((1 + NWAVE) * MROWS + 2 * MROWS * QS_TAIL_MAX_OUT + n_out * (n_layers ? R : 2 * R) + n_layers * R) * 4;
}

// colmax_store_acc (qs_policy_train.h) that folds into dst instead of overwriting it: the block's running maxima over
// the tiles it walks.  Every column has one writer (lane 16 or 48 of the wave that owns it), so no other thread's
// store is in the way.
template <int H>
__device__ __forceinline__ void colmax_fold_acc(float* dst, float4 (&m)[Geo<H>::CT][4], int wave, int lane) {
#pragma unroll
    for (int c = 0; c < Geo<H>::CT; ++c)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float v[4] = {m[c][g].x, m[c][g].y, m[c][g].z, m[c][g].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = fmaxf(v[j], dppf<0xB1>(v[j]));
                v[j] = fmaxf(v[j], dppf<0x4E>(v[j]));
                v[j] = fmaxf(v[j], dppf<0x124>(v[j]));
                v[j] = fmaxf(v[j], dppf<0x128>(v[j]));
                const int b = __builtin_bit_cast(int, v[j]);
                v[j] = fmaxf(v[j], __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(b, b, 0x142, 0xA, 0xF, false)));
            }
            if (lane == 16 || lane == 48) {
                const int n0 = acc_n0<H>(wave, c, g, lane);
#pragma unroll
                for (int j = 0; j < 4; ++j) dst[n0 + j] = fmaxf(dst[n0 + j], v[j]);
            }
        }
}

template <int R>
__global__ __launch_bounds__(NTHR, R == 128 ? 2 : 1) void policy_tail_bwd_x3_kernel(long B, int n_layers, TailTowers tw,
                                                                                    TailTrains trs) {
    constexpr int LDH = GeoX3<R>::LDH, CT = Geo<R>::CT, NO = QS_TAIL_MAX_OUT;
    constexpr float iSW = 1.f / X3_SW;
    constexpr size_t WBLK = (size_t)R * R / 4;   // uint4 per packed R x R block (hi + lo halves)
    extern __shared__ float4 smem4[];
    _Float16* gh = reinterpret_cast<_Float16*>(smem4);
    const TileX3 G{gh, gh + MROWS * LDH, LDH};
    const qs_tail_tower& t = tw.t[blockIdx.y];
    const qs_tail_train& tr = trs.t[blockIdx.y];
    const int n_out = t.n_out, Win = n_layers ? R : 2 * R;
    const bool actor = t.log_std != nullptr;
    float* RS = reinterpret_cast<float*>(gh + 2 * MROWS * LDH);   // 1 / s of the staged rows
    float* RMX = RS + MROWS;                                      // [NWAVE][MROWS] the waves' row maxima
    float* DO = RMX + NWAVE * MROWS;                              // [MROWS][NO] the head gradient dout
    float* LSD = DO + MROWS * NO;                                 // [MROWS][NO] the rows' log_std terms
    float* HW = LSD + MROWS * NO;                                 // [n_out][Win] the head's weights
    float* CM = HW + n_out * Win;                                 // [n_layers][R] running column maxima of |dpre_l|
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int e = tid; e < n_out * Win; e += NTHR) HW[e] = t.w_head[e];
    for (int e = tid; e < n_layers * R; e += NTHR) CM[e] = 0.f;
    // the block's partials over all its tiles: thread tid owns head columns tid and tid + 256 (every output), threads
    // < n_out the bias gradient and the log_std sum of output tid
    float hg[2][NO];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int o = 0; o < NO; ++o) hg[u][o] = 0.f;
    float hb = 0.f, hl = 0.f;
    const float* ylast = n_layers ? tr.y[n_layers - 1] : t.x;   // the head's input rows [B, Win]

    const long n_tiles = (B + MROWS - 1) / MROWS;
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long row0 = tile * MROWS;
        auto okrow = [&](int i) { return row0 + i < B; };
        __syncthreads();   // the previous tile's reads of DO, LSD, RS and the gradient tile (first tile: HW, CM)
        {   // the head gradient: four lanes per row, lane q outputs q and q + 4
            const int r = tid >> 2, q = tid & 3;
            const bool ok = okrow(r);
            const long row = ok ? row0 + r : 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int o = q + 4 * h;
                float d = 0.f, dl = 0.f;
                if (o < n_out) {
                    if (actor) {
                        const float up = tr.dlogp[row];
                        const float a = tr.actions[row * n_out + o], m = tr.mean[row * n_out + o], ls = t.log_std[o];
                        const float one = 1.f - 1.1920929e-07f;
                        const float y = fminf(fmaxf(a, -one), one);
                        const float g = 0.5f * (log1pf(y) - log1pf(-y));
                        const float e = expf(-ls);
                        const float z = (g - m) * e;
                        d = up * z * e;               // d log_prob / d mean_o
                        dl = up * (z * z - 1.f);      // d log_prob / d log_std_o
                    } else {
                        d = tr.dvalues[row * n_out + o];
                    }
                }
                DO[r * NO + o] = ok ? d : 0.f;
                LSD[r * NO + o] = ok ? dl : 0.f;
            }
            if (tid < MROWS) RS[tid] = X3_SW;   // the head's dy enters the chain unscaled: RS iSW = 1
        }
        __syncthreads();
        if (tid < 64) {   // the rows' sums per output: lane (part, o) eight rows, the parts through the wave
            const int o = tid & 7, r0 = tid & ~7;
            float sb = 0.f, sl = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                sb += DO[(r0 + j) * NO + o];
                sl += LSD[(r0 + j) * NO + o];
            }
#pragma unroll
            for (int x = 8; x < 64; x <<= 1) {
                sb += __shfl_xor(sb, x);
                sl += __shfl_xor(sl, x);
            }
            hb += sb;   // (kept by the threads < n_out)
            hl += sl;
        }
        // head weight gradient: sum_r dout[r][o] y_L[r][k] for the thread's columns k (coalesced row loads, eight in flight)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int k = tid + u * NTHR;
            if (k < Win) {
#pragma nounroll
                for (int r0 = 0; r0 < MROWS; r0 += 8) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = ylast[(okrow(r0 + j) ? row0 + r0 + j : 0) * (long)Win + k];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float4 d0 = lds4(DO + (r0 + j) * NO), d1 = lds4(DO + (r0 + j) * NO + 4);
                        const float d[NO] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
                        for (int o = 0; o < NO; ++o)
                            if (o < n_out) hg[u][o] = fmaf(d[o], v[j], hg[u][o]);   // (uniform)
                    }
                }
            }
        }
        if (n_layers == 0) {   // dlat is the head's dy: dout W_head over the 2R input columns
            constexpr int W4 = 2 * R / 4;
            for (int e = tid; e < MROWS * W4; e += NTHR) {
                const int r = e / W4, c4 = e - r * W4;
                if (!okrow(r)) continue;
                const float4 d0 = lds4(DO + r * NO), d1 = lds4(DO + r * NO + 4);
                const float d[NO] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
                float4 s = z4;
#pragma unroll
                for (int o = 0; o < NO; ++o)
                    if (o < n_out) {
                        const float4 w = lds4(HW + o * Win + 4 * c4);
                        s.x = fmaf(d[o], w.x, s.x); s.y = fmaf(d[o], w.y, s.y);
                        s.z = fmaf(d[o], w.z, s.z); s.w = fmaf(d[o], w.w, s.w);
                    }
                st4g(tr.dlat + (row0 + r) * (long)(2 * R) + 4 * c4, s);
            }
            continue;
        }

        // the chain: the gradient stays in the accumulator registers from the head's dy to dlat
        f32x16 acc[RT][CT];
        float4 aux[RT][CT][4];
        load_acc_rows<R>(tr.y[n_layers - 1], row0, okrow, wave, lane, aux);
        // dy_L = dout W_head at the lane's accumulator positions, one output at a time (its weights read once for both
        // row tiles; unrolled over the outputs, the 128 LDS reads are hoisted into as many registers)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[rt][c][j] = 0.f;
#pragma nounroll
        for (int o = 0; o < n_out; ++o) {
            float d[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) d[rt] = DO[acc_i(rt, lane) * NO + o];
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 w = lds4(HW + o * R + acc_n0<R>(wave, c, g, lane));
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        acc[rt][c][4 * g] = fmaf(d[rt], w.x, acc[rt][c][4 * g]);
                        acc[rt][c][4 * g + 1] = fmaf(d[rt], w.y, acc[rt][c][4 * g + 1]);
                        acc[rt][c][4 * g + 2] = fmaf(d[rt], w.z, acc[rt][c][4 * g + 2]);
                        acc[rt][c][4 * g + 3] = fmaf(d[rt], w.w, acc[rt][c][4 * g + 3]);
                    }
                }
        }
#pragma nounroll
        for (int l = n_layers - 1; l >= 0; --l) {
            const uint4* wt = reinterpret_cast<const uint4*>(tr.w_chain_t[l]);
            WQueue<R> q = mfma_prefetch_x3<R>(wt, wave, lane);   // ahead of dpre_l's stores
            float* dp = tr.dpre[l];
            float4 cma[CT][4];
            // dpre_l = dy_l (1 - y_l^2): stored, its column maxima, and staged at the rows' scales (the barrier inside
            // follows every wave's last read of the tile)
            stage_acc_scaled<R>(G, acc, RS, RMX, wave, lane, aux, [&](int i, int n0, float4 a, float4 y) {
                if (!okrow(i)) return z4;
                const float4 v = f4_dtanh(f4_scale(a, RS[i] * iSW), y);
                st4g(dp + (row0 + i) * R + n0, v);
                return v;
            }, cma);
            colmax_fold_acc<R>(CM + l * R, cma, wave, lane);
            __syncthreads();
            if (l > 0) {
                load_acc_rows<R>(tr.y[l - 1], row0, okrow, wave, lane, aux);   // in flight during the layer's MFMAs
                mfma_layer_x3<R, R>(G, wt, acc, wave, lane, q);                // dy_{l-1} s_i s_w
            } else {
#pragma nounroll
                for (int h = 0; h < 2; ++h) {   // the two R x R blocks of W_0^T on the same staged tile
                    if (h) q = mfma_prefetch_x3<R>(wt + WBLK, wave, lane);
                    mfma_layer_x3<R, R>(G, wt + h * WBLK, acc, wave, lane, q);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        const int i = acc_i(rt, lane);
                        if (!okrow(i)) continue;
                        const float sc = RS[i] * iSW;
#pragma unroll
                        for (int c = 0; c < CT; ++c)
#pragma unroll
                            for (int g = 0; g < 4; ++g)
                                st4g(tr.dlat + (row0 + i) * (long)(2 * R) + h * R + acc_n0<R>(wave, c, g, lane),
                                     f4_scale(acc4(acc[rt][c], g), sc));
                    }
                }
            }
        }
    }

    // the block's partials, once
    float* hp = tr.head_part + (size_t)blockIdx.x * n_out * (Win + 1);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int k = tid + u * NTHR;
        if (k < Win) {
#pragma unroll
            for (int o = 0; o < NO; ++o)
                if (o < n_out) hp[o * (Win + 1) + k] = hg[u][o];
        }
    }
    if (tid < n_out) {
        hp[tid * (Win + 1) + Win] = hb;
        if (actor) tr.log_std_part[(size_t)blockIdx.x * n_out + tid] = hl;
    }
    __syncthreads();   // CM: the last tile's folds
    for (int e = tid; e < n_layers * R; e += NTHR) {
        const int l = e / R, n = e - l * R;
        tr.colmax[((size_t)l * gridDim.x + blockIdx.x) * R + n] = CM[e];
    }
}

}  // namespace pol
}  // namespace qs
