// qs_policy_api.hip -- the C ABI (include/quadswarm.h) over the policy kernels: the rollout's fused attention
// encoders (qs_policy.h, qs_policy_x3.h) and the PPO update's encoder forward / backward, weight gradients and column
// statistics (qs_policy_train.h).  Its own translation unit: the env step kernels (qs_step.hip) and these build and
// rebuild independently into the same libquadswarm.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>

#include "quadswarm.h"
#include "qs_common.h"
#include "qs_policy_train.h"
#include "qs_policy.h"
#include "qs_policy_x3.h"
#include "qs_error.h"

static int fail(int code, const std::string& msg) { return qs_fail(code, msg); }
#define QS_HIP(call) QS_HIP_CHECK(call)

#ifdef QS_STAMPS
// the policy kernels' phase stamps (this translation unit's copy of qs_dbg_stamps; tools/policy_stamps.py)
extern "C" int qs_debug_stamps_policy(uint64_t* host, size_t n) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(qs::qs_dbg_stamps), n * sizeof(uint64_t)) == hipSuccess ? 0 : -3;
}
#endif

// a kernel that uses dynamic LDS: raise its limit to lds bytes, launch, report a launch error
template <typename Kernel, typename... Args>
static int launch_lds(Kernel kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    QS_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    QS_HIP(hipGetLastError());
    return QS_OK;
}
// f(std::integral_constant<int, H>) for the hidden size H, which the caller has checked to be 128 or 256
template <typename F>
static int with_H(int32_t H, F f) {
    return H == 256 ? f(std::integral_constant<int, 256>()) : f(std::integral_constant<int, 128>());
}

// The attention encoder's row-block kernels: the rollout's forward (qs_policy.h, or qs_policy_x3.h with x3) and the
// PPO update's forward with saves and backward (qs_policy_train.h, which take the towers' qs_attn_train too).
enum { ST_EMBED, ST_POOL, ST_EMBED_TRAIN, ST_POOL_TRAIN, ST_BWD1, ST_BWD2 };
static int attn_check(int32_t B, int32_t K, int32_t H, const qs_attn_tower* towers, int32_t n_towers) {
    if (!towers) return fail(QS_E_INVALID, "NULL towers");
    if (n_towers < 1 || n_towers > QS_ATTN_MAX_TOWERS) return fail(QS_E_INVALID, "n_towers must be 1 or 2");
    if (H != 128 && H != 256) return fail(QS_E_INVALID, "attention hidden size must be 128 or 256");
    if (K < 1 || K > qs::pol::MROWS) return fail(QS_E_INVALID, "neighbours per agent must be 1..64");
    if (B < 1) return fail(QS_E_INVALID, "B must be >= 1");
    if ((long long)B * K * H >= (1ll << 31)) return fail(QS_E_INVALID, "B * K * H must stay below 2^31");
    return QS_OK;
}
// (obs, stride, so, off, nd: the embedding stages' observation block; trains: the update's stages)
static int attn_impl(int stage, bool x3, const float* obs, int32_t stride, int32_t so, int32_t off, int32_t B,
                     int32_t K, int32_t nd, int32_t H, const qs_attn_tower* towers, const qs_attn_train* trains,
                     int32_t n_towers, void* stream) {
    namespace P = qs::pol;
    int rc = attn_check(B, K, H, towers, n_towers);
    if (rc) return rc;
    const bool train = stage != ST_EMBED && stage != ST_POOL;
    if (train && !trains) return fail(QS_E_INVALID, "NULL trains");
    if (stage == ST_EMBED || stage == ST_EMBED_TRAIN) {
        if (!obs) return fail(QS_E_INVALID, "NULL obs");
        if (nd < 1 || nd > P::MAX_ND) return fail(QS_E_INVALID, "features per neighbour must be 1..16");
        if (so < 1 || so > stride) return fail(QS_E_INVALID, "self features must lie inside the obs row");
        if (nd + so > P::KD0) return fail(QS_E_INVALID, "self + neighbour features must be <= 32");
        if (off < 0 || off + K * nd > stride) return fail(QS_E_INVALID, "neighbour block outside the obs row");
    }
    P::Towers tw{};
    P::Trains trs{};
    for (int i = 0; i < n_towers; ++i) {
        const qs_attn_tower& t = towers[i];
        const qs_attn_train r = train ? trains[i] : qs_attn_train{};
        bool ok = true;
        const char* what = "NULL tower / train pointer for this stage";
        switch (stage) {
            case ST_EMBED:
                ok = t.w_e1p && t.b_e1 && t.w_e2p && t.b_e2 && t.e2 && t.e_mean;
                what = "NULL stage-1 tower pointer";
                break;
            case ST_POOL:
                ok = t.e2 && t.P && t.w_v1p && t.b_v1 && t.w_v2p && t.b_v2 && t.w_a1ep && t.w_a2p && t.b_a2 && t.w_a3 &&
                     t.out;
                what = "NULL stage-2 tower pointer";
                break;
            case ST_EMBED_TRAIN: ok = t.w_e1p && t.b_e1 && t.w_e2p && t.b_e2 && t.e2 && t.e_mean && r.e1; break;
            case ST_POOL_TRAIN:
                ok = t.e2 && t.P && t.w_v1p && t.b_v1 && t.w_v2p && t.b_v2 && t.w_a1ep && t.w_a2p && t.b_a2 && t.w_a3 &&
                     t.out && r.a1 && r.a2 && r.v1 && r.h && r.w;
                break;
            case ST_BWD1:
                ok = t.w_a3 && r.w && r.h && r.v1 && r.a1 && r.a2 && r.dout && r.w_v2tp && r.w_v1tp && r.w_a2tp &&
                     r.w_a1etp && r.dh_pre && r.dv1_pre && r.da2_pre && r.da1_pre && r.dscore && r.de2p;
                break;
            default: ok = t.e2 && r.e1 && r.de2p && r.dem && r.w_e2tp && r.de2_pre && r.de1_pre; break;
        }
        if (!ok) return fail(QS_E_INVALID, what);
        tw.t[i] = t;
        trs.t[i] = r;
    }
    const int mu = (P::MROWS / K) * K;   // a block's rows: whole agents
    const dim3 grid((unsigned)(((long long)B * K + mu - 1) / mu), (unsigned)n_towers), block(P::NTHR);
    hipStream_t st = (hipStream_t)stream;
    return with_H(H, [&](auto h) {
        constexpr int HH = decltype(h)::value;
        switch (stage) {
            case ST_EMBED:
                return x3 ? launch_lds(P::attn_embed_x3_kernel<HH>, grid, block, P::embed_x3_lds_bytes<HH>(), st, obs, stride,
                                       so, off, B, K, nd, tw)
                          : launch_lds(P::attn_embed_kernel<HH>, grid, block, P::embed_lds_bytes<HH>(), st, obs, stride, so,
                                       off, B, K, nd, tw);
            case ST_POOL:
                return x3 ? launch_lds(P::attn_pool_x3_kernel<HH>, grid, block, P::pool_x3_lds_bytes<HH>(), st, B, K, tw)
                          : launch_lds(P::attn_pool_kernel<HH>, grid, block, P::pool_lds_bytes<HH>(), st, B, K, tw);
            case ST_EMBED_TRAIN:
                return launch_lds(P::attn_embed_train_x3_kernel<HH>, grid, block, P::embed_x3_lds_bytes<HH>(), st, obs,
                                  stride, so, off, B, K, nd, tw, trs);
            case ST_POOL_TRAIN:
                return launch_lds(P::attn_pool_train_x3_kernel<HH>, grid, block, P::pool_x3_lds_bytes<HH>(), st, B, K, tw, trs);
            case ST_BWD1:
                return launch_lds(P::attn_bwd1_x3_kernel<HH>, grid, block, P::bwd1_lds_bytes<HH>(K), st, B, K, tw, trs);
            default:
                return launch_lds(P::attn_bwd2_x3_kernel<HH>, grid, block, P::bwd2_lds_bytes<HH>(), st, B, K, tw, trs);
        }
    });
}
extern "C" int qs_attn_embed(const float* obs, int32_t obs_stride, int32_t self_dim, int32_t nbr_off, int32_t B,
                             int32_t K, int32_t nd, int32_t H, const qs_attn_tower* towers, int32_t n_towers,
                             void* stream) {
    return attn_impl(ST_EMBED, false, obs, obs_stride, self_dim, nbr_off, B, K, nd, H, towers, nullptr, n_towers, stream);
}
extern "C" int qs_attn_embed_x3(const float* obs, int32_t obs_stride, int32_t self_dim, int32_t nbr_off, int32_t B,
                                int32_t K, int32_t nd, int32_t H, const qs_attn_tower* towers, int32_t n_towers,
                                void* stream) {
    return attn_impl(ST_EMBED, true, obs, obs_stride, self_dim, nbr_off, B, K, nd, H, towers, nullptr, n_towers, stream);
}
extern "C" int qs_attn_pool(int32_t B, int32_t K, int32_t H, const qs_attn_tower* towers, int32_t n_towers,
                            void* stream) {
    return attn_impl(ST_POOL, false, nullptr, 0, 0, 0, B, K, 0, H, towers, nullptr, n_towers, stream);
}
extern "C" int qs_attn_pool_x3(int32_t B, int32_t K, int32_t H, const qs_attn_tower* towers, int32_t n_towers,
                               void* stream) {
    return attn_impl(ST_POOL, true, nullptr, 0, 0, 0, B, K, 0, H, towers, nullptr, n_towers, stream);
}
extern "C" int qs_attn_embed_train_x3(const float* obs, int32_t obs_stride, int32_t self_dim, int32_t nbr_off, int32_t B,
                                      int32_t K, int32_t nd, int32_t H, const qs_attn_tower* towers,
                                      const qs_attn_train* trains, int32_t n_towers, void* stream) {
    return attn_impl(ST_EMBED_TRAIN, true, obs, obs_stride, self_dim, nbr_off, B, K, nd, H, towers, trains, n_towers, stream);
}
extern "C" int qs_attn_pool_train_x3(int32_t B, int32_t K, int32_t H, const qs_attn_tower* towers,
                                     const qs_attn_train* trains, int32_t n_towers, void* stream) {
    return attn_impl(ST_POOL_TRAIN, true, nullptr, 0, 0, 0, B, K, 0, H, towers, trains, n_towers, stream);
}
extern "C" int qs_attn_bwd1_x3(int32_t B, int32_t K, int32_t H, const qs_attn_tower* towers,
                               const qs_attn_train* trains, int32_t n_towers, void* stream) {
    return attn_impl(ST_BWD1, true, nullptr, 0, 0, 0, B, K, 0, H, towers, trains, n_towers, stream);
}
extern "C" int qs_attn_bwd2_x3(int32_t B, int32_t K, int32_t H, const qs_attn_tower* towers,
                               const qs_attn_train* trains, int32_t n_towers, void* stream) {
    return attn_impl(ST_BWD2, true, nullptr, 0, 0, 0, B, K, 0, H, towers, trains, n_towers, stream);
}

// the update's weight gradients: dW = G^T A over n_parts row ranges (qs_policy_train.h dw_x3_kernel, dw0_x3_kernel)
extern "C" int qs_dw_x3_ld(const float* G, int32_t ldg, const float* A, int32_t lda, const float* col_scale, int64_t R,
                           int32_t H, float* part, float* part_sum, int32_t n_parts, void* stream) {
    namespace P = qs::pol;
    if (!G || !A || !col_scale || !part) return fail(QS_E_INVALID, "NULL argument");
    if (H != 128 && H != 256) return fail(QS_E_INVALID, "hidden size must be 128 or 256");
    if (ldg < H || lda < H || ldg > 4096 || lda > 4096) return fail(QS_E_INVALID, "row strides H .. 4096 floats");
    if (R < 1 || n_parts < 1 || n_parts > 65535 || R * (int64_t)(ldg > lda ? ldg : lda) >= (1ll << 40))
        return fail(QS_E_INVALID, "R >= 1, 1 <= n_parts <= 65535");
    const long long rows_per = (R + n_parts - 1) / n_parts;
    const int steps = (int)((rows_per + P::DW_STEP - 1) / P::DW_STEP);
    if ((long long)steps * P::DW_STEP * (ldg > lda ? ldg : lda) * 4 >= (1ll << 31))
        return fail(QS_E_INVALID, "rows per part x row stride too large (use more parts)");
    return with_H(H, [&](auto h) {
        constexpr int HH = decltype(h)::value;
        return launch_lds(P::dw_x3_kernel<HH>, dim3((unsigned)n_parts), dim3(P::dw_threads<HH>()), P::dw_lds_bytes<HH>(),
                          (hipStream_t)stream, G, A, col_scale, (long)R, steps, part, part_sum, (int)ldg, (int)lda);
    });
}
extern "C" int qs_attn_dw_x3(const float* G, const float* A, const float* col_scale, int64_t R, int32_t H, float* part,
                             float* part_sum, int32_t n_parts, void* stream) {
    return qs_dw_x3_ld(G, H, A, H, col_scale, R, H, part, part_sum, n_parts, stream);
}
extern "C" int qs_attn_dw0_x3(const float* G, const float* col_scale, const float* obs, int32_t stride, int32_t so,
                              int32_t off, int32_t B, int32_t K, int32_t nd, int32_t H, float* part, float* part_sum,
                              int32_t n_parts, void* stream) {
    namespace P = qs::pol;
    if (!G || !col_scale || !obs || !part) return fail(QS_E_INVALID, "NULL argument");
    if (H != 128 && H != 256) return fail(QS_E_INVALID, "hidden size must be 128 or 256");
    if (B < 1 || K < 1 || (int64_t)B * K >= (1ll << 31) || n_parts < 1 || n_parts > 65535)
        return fail(QS_E_INVALID, "B, K >= 1, B K < 2^31, 1 <= n_parts <= 65535");
    if (nd < 0 || so < 1 || nd + so > P::KD0) return fail(QS_E_INVALID, "nd >= 0, self_dim >= 1, nd + self_dim <= 32");
    if (so > stride || off < 0 || off + (int64_t)K * nd > stride)
        return fail(QS_E_INVALID, "self features and the neighbour block must lie inside the obs row");
    const long long R = (long long)B * K;
    const long long rows_per = (R + n_parts - 1) / n_parts;
    const int steps = (int)((rows_per + P::DW_STEP - 1) / P::DW_STEP);
    return with_H(H, [&](auto h) {
        constexpr int HH = decltype(h)::value;
        return launch_lds(P::dw0_x3_kernel<HH>, dim3((unsigned)n_parts), dim3(P::NTHR), P::dw0_lds_bytes<HH>(),
                          (hipStream_t)stream, G, col_scale, obs, stride, so, off, B, K, nd, (long)R, steps, part, part_sum);
    });
}

// Y = X W^T on the split-f16 matrix cores (qs_policy_x3.h linear_tanh_x3_kernel), K = 256 or 512 input columns read
// as 256-column slices: slice 0 from X, slice 1 from X1, rows ldx floats apart.  ROWS: the backward's dX with per-row
// scales (no bias); else + bias, and tanh if ACT.
template <bool ROWS, bool ACT>
static int linear_x3(const float* X, const float* X1, int64_t ldx, int64_t M, int32_t K, const void* w_packed,
                     int64_t w_bytes, const float* bias, const float* row_scale, float* Y, int32_t N, void* stream) {
    namespace P = qs::pol;
    const bool cat = ldx != K;   // qs_linear_tanh_cat_x3: two [M, 256] inputs, no K of the caller's
    if (!X || !X1 || !w_packed || !(ROWS ? row_scale : bias) || !Y) return fail(QS_E_INVALID, "NULL argument");
    if (M < 1 || M >= (1ll << 31) / 512 || (K != 256 && K != 512) || N < 256 || N > 1024 || N % 256)
        return fail(QS_E_INVALID, cat ? "M >= 1, N a multiple of 256 up to 1024"
                                      : "M >= 1, K 256 or 512, N a multiple of 256 up to 1024");
    // the packed operand: (N / 256) (K / 256) blocks of 256 x 256 weights as f16 hi + lo halves
    if (w_bytes != (int64_t)(N / 256) * (K / 256) * 256 * 256 * 2 * 2)
        return fail(QS_E_INVALID, cat ? "w_bytes: the packed weight must hold (N / 256) 2 packed 256 x 256 blocks"
                                      : "w_bytes: the packed weight must hold (N / 256) (K / 256) packed 256 x 256 blocks");
    const dim3 grid((unsigned)((M + P::MROWS - 1) / P::MROWS), (unsigned)(N / 256)), block(P::NTHR);
    const uint4* wp = reinterpret_cast<const uint4*>(w_packed);
    hipStream_t st = (hipStream_t)stream;
    return K == 256 ? launch_lds(P::linear_tanh_x3_kernel<1, ROWS, ACT>, grid, block, P::linear_x3_lds_bytes(), st, X, X1,
                                 (long)ldx, (long)M, wp, bias, Y, N, row_scale)
                    : launch_lds(P::linear_tanh_x3_kernel<2, ROWS, ACT>, grid, block, P::linear_x3_lds_bytes(), st, X, X1,
                                 (long)ldx, (long)M, wp, bias, Y, N, row_scale);
}
extern "C" int qs_linear_tanh_x3(const float* X, int64_t M, int32_t K, const void* w_packed, int64_t w_bytes,
                                 const float* bias, float* Y, int32_t N, void* stream) {
    return linear_x3<false, true>(X, X + 256, K, M, K, w_packed, w_bytes, bias, nullptr, Y, N, stream);
}
extern "C" int qs_linear_tanh_cat_x3(const float* X0, const float* X1, int64_t M, const void* w_packed, int64_t w_bytes,
                                     const float* bias, float* Y, int32_t N, void* stream) {
    return linear_x3<false, true>(X0, X1, 256, M, 512, w_packed, w_bytes, bias, nullptr, Y, N, stream);
}
extern "C" int qs_linear_rows_x3(const float* X, const float* row_scale, int64_t M, int32_t K, const void* w_packed,
                                 int64_t w_bytes, float* Y, int32_t N, void* stream) {
    return linear_x3<true, true>(X, X + 256, K, M, K, w_packed, w_bytes, nullptr, row_scale, Y, N, stream);
}
extern "C" int qs_linear_bias_x3(const float* X, int64_t M, int32_t K, const void* w_packed, int64_t w_bytes,
                                 const float* bias, float* Y, int32_t N, void* stream) {
    return linear_x3<false, false>(X, X + 256, K, M, K, w_packed, w_bytes, bias, nullptr, Y, N, stream);
}

// the update's row / column statistics (qs_policy_train.h; no dynamic LDS)
extern "C" int qs_tanh_grad_stats(const float* g, const float* y, float* gp, float* row_scale, float* col_part, int64_t M,
                                  int32_t N, void* stream) {
    namespace P = qs::pol;
    if (!g || !y || !gp || !row_scale || !col_part) return fail(QS_E_INVALID, "NULL argument");
    if (M < 1 || M >= (1ll << 31) / 512 || (N != 256 && N != 512)) return fail(QS_E_INVALID, "M >= 1, N 256 or 512");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((M + P::MROWS - 1) / P::MROWS));
    if (N == 256)
        hipLaunchKernelGGL(P::tanh_grad_stats_kernel<1>, grid, dim3(P::NTHR), 0, st, g, y, gp, row_scale, col_part, (long)M);
    else
        hipLaunchKernelGGL(P::tanh_grad_stats_kernel<2>, grid, dim3(P::NTHR), 0, st, g, y, gp, row_scale, col_part, (long)M);
    QS_HIP(hipGetLastError());
    return QS_OK;
}
extern "C" int qs_slab_sum_stats(const float* G, int32_t n_slabs, int64_t M, int32_t N, float* out, float* row_scale,
                                 float* col_part, void* stream) {
    namespace P = qs::pol;
    if (!G || !out || !row_scale || !col_part) return fail(QS_E_INVALID, "NULL argument");
    if (n_slabs < 1 || M < 1 || (int64_t)n_slabs * M >= (1ll << 31) / 512 || (N != 256 && N != 512))
        return fail(QS_E_INVALID, "n_slabs >= 1, M >= 1, n_slabs M < 2^22, N 256 or 512");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((M + P::MROWS - 1) / P::MROWS));
    if (N == 256)
        hipLaunchKernelGGL(P::slab_sum_stats_kernel<1>, grid, dim3(P::NTHR), 0, st, G, (int)n_slabs, out, row_scale, col_part,
                           (long)M);
    else
        hipLaunchKernelGGL(P::slab_sum_stats_kernel<2>, grid, dim3(P::NTHR), 0, st, G, (int)n_slabs, out, row_scale, col_part,
                           (long)M);
    QS_HIP(hipGetLastError());
    return QS_OK;
}
extern "C" int qs_colmax_reduce(const float* part_max, int32_t n_stats, int32_t n_blocks, int32_t H, float* out,
                                void* stream) {
    namespace P = qs::pol;
    if (!part_max || !out) return fail(QS_E_INVALID, "NULL argument");
    if (n_stats < 1 || n_stats > QS_ATTN_NCOLMAX || n_blocks < 1 || H < 1 || H > 4096)
        return fail(QS_E_INVALID, "1 <= n_stats <= QS_ATTN_NCOLMAX, n_blocks >= 1, 1 <= H <= 4096");
    hipStream_t st = (hipStream_t)stream;
    QS_HIP(hipMemsetAsync(out, 0, (size_t)n_stats * H * sizeof(float), st));
    hipLaunchKernelGGL(P::colmax_reduce_kernel, dim3(P::CM_CHUNKS, (unsigned)((H + 63) / 64), (unsigned)n_stats),
                       dim3(256), 0, st, part_max, n_blocks, H, out);
    QS_HIP(hipGetLastError());
    return QS_OK;
}
extern "C" int qs_colstats(const float* G, int64_t R, int32_t H, const float* row_w, const float* obs, int32_t stride,
                           int32_t nbr_off, int32_t B, int32_t K, int32_t nd, int32_t nx, float* pmx, float* psm,
                           float* px, int32_t n_parts, void* stream) {
    namespace P = qs::pol;
    if (!G || !pmx || !psm) return fail(QS_E_INVALID, "NULL argument");
    if (H != 128 && H != 256) return fail(QS_E_INVALID, "hidden size must be 128 or 256");
    if (R < 1 || n_parts < 1 || n_parts > (1 << 24) || R * (int64_t)H >= (1ll << 40))
        return fail(QS_E_INVALID, "R >= 1, 1 <= n_parts <= 2^24");
    if (nx < 0 || nx > QS_COLSTATS_MAX_X) return fail(QS_E_INVALID, "nx out of range");
    if (nx > 0 && (!obs || !px || B < 1 || K < 1 || nd < 0 || nd > nx || (int64_t)B * K != R || R >= (1ll << 31) ||
                   stride < nx ||
                   nbr_off < 0 || nbr_off + (int64_t)K * nd > stride))
        return fail(QS_E_INVALID, "layer-0 input: obs, part_x, B K = R, nd <= nx, the neighbour block inside a row");
    hipStream_t st = (hipStream_t)stream;
    const long rows_per = (long)((R + n_parts - 1) / n_parts);
    if (nx > 8)
        hipLaunchKernelGGL(P::colstats_kernel<QS_COLSTATS_MAX_X>, dim3((unsigned)n_parts), dim3(H), 0, st, G, (long)R, H,
                           rows_per, row_w, obs, stride, nbr_off, B, K, nd, nx, pmx, psm, px);
    else if (nx > 0)   // the neighbour features alone (nd <= 8)
        hipLaunchKernelGGL(P::colstats_kernel<8>, dim3((unsigned)n_parts), dim3(H), 0, st, G, (long)R, H, rows_per, row_w,
                           obs, stride, nbr_off, B, K, nd, nx, pmx, psm, px);
    else
        hipLaunchKernelGGL(P::colstats_kernel<0>, dim3((unsigned)n_parts), dim3(H), 0, st, G, (long)R, H, rows_per,
                           row_w, obs, stride, nbr_off, B > 0 ? B : 1, K > 0 ? K : 1, nd, 0, pmx, psm, px);
    QS_HIP(hipGetLastError());
    return QS_OK;
}
