// qs_policy_enc_train.hip -- the C ABI (include/quadswarm.h qs_encoder_mlp_train_x3, qs_encoder_mlp_bwd_x3) over the PPO
// update's MLP-family encoder kernels (qs_policy_enc_train.h).  Its own translation unit, built like qs_policy_enc.hip
// with the packed fp32 VALU instructions off (Makefile MHA_FLAGS); of qs_policy_train.h it takes the staging helpers only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "quadswarm.h"
#include "qs_common.h"
#define QS_TRAIN_STAGING_ONLY 1
#include "qs_policy_enc_train.h"
#include "qs_error.h"

namespace P = qs::pol;

// qs_encoder_mlp_x3's checks plus the train structs'; fills tw / trs
static int enc_train_args(const float* obs, int32_t obs_stride, int32_t self_dim, int32_t nbr_kind, int32_t K,
                          int32_t nbr_dim, int32_t obst_dim, int32_t B, int32_t H, const qs_enc_tower* towers,
                          const qs_enc_train* trains, int32_t n_towers, bool backward, P::EncTowers& tw, P::EncTrains& trs) {
    if (!obs || !towers || !trains) return qs_fail(QS_E_INVALID, "NULL argument");
    if (n_towers < 1 || n_towers > QS_ATTN_MAX_TOWERS) return qs_fail(QS_E_INVALID, "n_towers must be 1 or 2");
    if (H != 128 && H != 256) return qs_fail(QS_E_INVALID, "hidden size must be 128 or 256");
    if (nbr_kind != QS_ENC_NBR_NONE && nbr_kind != QS_ENC_NBR_MEAN && nbr_kind != QS_ENC_NBR_MLP)
        return qs_fail(QS_E_INVALID, "nbr_kind must be a qs_enc_nbr_kind");
    if (self_dim < 1 || self_dim > P::ENC_SW) return qs_fail(QS_E_INVALID, "self features must be 1..32");
    if (K < 0 || K > 4096 || nbr_dim < 0 || nbr_dim > 4096)
        return qs_fail(QS_E_INVALID, "K and nbr_dim must be 0..4096");
    if (nbr_kind == QS_ENC_NBR_MLP && (K * nbr_dim < 1 || K * nbr_dim > P::ENC_NBW))
        return qs_fail(QS_E_INVALID, "mlp neighbour block K * nbr_dim must be 1..64 wide");
    if (nbr_kind == QS_ENC_NBR_MEAN && (K < 1 || nbr_dim < 1 || nbr_dim > P::ENC_NDW))
        return qs_fail(QS_E_INVALID, "mean_embed needs K >= 1 and 1..16 features per neighbour");
    if (obst_dim < 0 || obst_dim > P::ENC_OBW) return qs_fail(QS_E_INVALID, "obstacle values must be 0..16");
    if ((long long)self_dim + (long long)K * nbr_dim + obst_dim > obs_stride)
        return qs_fail(QS_E_INVALID, "the self, neighbour and obstacle values must lie inside the obs row");
    if (B < 1 || (long long)B * (obs_stride > 2 * H ? obs_stride : 2 * H) >= (1ll << 31))
        return qs_fail(QS_E_INVALID, "B >= 1, B * max(obs_stride, 2 H) below 2^31");
    for (int i = 0; i < n_towers; ++i) {
        const qs_enc_tower& t = towers[i];
        const qs_enc_train& r = trains[i];
        bool ok = t.w_s1p && t.b_s1 && t.w_s2p && t.b_s2 && t.w_ffp && t.b_ff && t.out;
        if (nbr_kind != QS_ENC_NBR_NONE) ok = ok && t.w_n1p && t.b_n1 && t.w_n2p && t.b_n2;
        if (nbr_kind == QS_ENC_NBR_MLP) ok = ok && t.w_n3p && t.b_n3;
        if (obst_dim > 0) ok = ok && t.w_o1p && t.b_o1 && t.w_o2p && t.b_o2;
        if (!ok) return qs_fail(QS_E_INVALID, "NULL tower pointer");
        ok = r.s1 && r.s2;
        if (nbr_kind != QS_ENC_NBR_NONE) ok = ok && r.n1 && r.n2;
        if (nbr_kind == QS_ENC_NBR_MLP) ok = ok && r.n3;
        if (nbr_kind == QS_ENC_NBR_MEAN) ok = ok && r.m;
        if (obst_dim > 0) ok = ok && r.o1 && r.o2;
        if (backward) {
            ok = ok && r.dout && r.dpre_ff && r.dpre_s1 && r.dpre_s2 && r.colmax && r.w_s2t && r.w_fft;
            if (nbr_kind != QS_ENC_NBR_NONE) ok = ok && r.dpre_n1 && r.dpre_n2 && r.w_n2t;
            if (nbr_kind == QS_ENC_NBR_MLP) ok = ok && r.dpre_n3 && r.w_n3t;
            if (nbr_kind == QS_ENC_NBR_MEAN) ok = ok && r.dm;
            if (obst_dim > 0) ok = ok && r.dpre_o1 && r.dpre_o2 && r.w_o2t;
        }
        if (!ok) return qs_fail(QS_E_INVALID, "NULL train pointer");
        tw.t[i] = t;
        trs.t[i] = r;
    }
    return QS_OK;
}

template <typename K, typename... A>
static int launch_enc_train(K kernel, dim3 grid, size_t lds, hipStream_t st, A... a) {
    QS_HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, grid, dim3(P::NTHR), lds, st, a...);
    QS_HIP_CHECK(hipGetLastError());
    return QS_OK;
}

template <int H>
static int launch_fwd(int32_t kind, dim3 grid, hipStream_t st, const float* obs, int32_t stride, int32_t so, int32_t K,
                      int32_t nd, int32_t od, int32_t B, const P::EncTowers& tw, const P::EncTrains& trs) {
    const size_t lds = P::enc_lds_bytes<H>();
    switch (kind) {
        case QS_ENC_NBR_MEAN:
            return launch_enc_train(P::enc_mlp_train_x3_kernel<H, QS_ENC_NBR_MEAN>, grid, lds, st, obs, stride, so, K, nd, od, B, tw, trs);
        case QS_ENC_NBR_MLP:
            return launch_enc_train(P::enc_mlp_train_x3_kernel<H, QS_ENC_NBR_MLP>, grid, lds, st, obs, stride, so, K, nd, od, B, tw, trs);
        default:
            return launch_enc_train(P::enc_mlp_train_x3_kernel<H, QS_ENC_NBR_NONE>, grid, lds, st, obs, stride, so, K, nd, od, B, tw, trs);
    }
}

template <int H>
static int launch_bwd(int32_t kind, dim3 grid, hipStream_t st, int32_t K, int32_t od, int32_t B, const P::EncTowers& tw,
                      const P::EncTrains& trs) {
    const size_t lds = P::enc_bwd_lds_bytes<H>();
    switch (kind) {
        case QS_ENC_NBR_MEAN: return launch_enc_train(P::enc_mlp_bwd_x3_kernel<H, QS_ENC_NBR_MEAN>, grid, lds, st, K, od, B, tw, trs);
        case QS_ENC_NBR_MLP: return launch_enc_train(P::enc_mlp_bwd_x3_kernel<H, QS_ENC_NBR_MLP>, grid, lds, st, K, od, B, tw, trs);
        default: return launch_enc_train(P::enc_mlp_bwd_x3_kernel<H, QS_ENC_NBR_NONE>, grid, lds, st, K, od, B, tw, trs);
    }
}

// 64 agents per block, one grid row per tower (the rollout kernel's geometry)
extern "C" int qs_encoder_mlp_train_x3(const float* obs, int32_t obs_stride, int32_t self_dim, int32_t nbr_kind, int32_t K,
                                       int32_t nbr_dim, int32_t obst_dim, int32_t B, int32_t H, const qs_enc_tower* towers,
                                       const qs_enc_train* trains, int32_t n_towers, void* stream) {
    P::EncTowers tw{};
    P::EncTrains trs{};
    if (int rc = enc_train_args(obs, obs_stride, self_dim, nbr_kind, K, nbr_dim, obst_dim, B, H, towers, trains, n_towers,
                                false, tw, trs))
        return rc;
    const dim3 grid((unsigned)((B + P::MROWS - 1) / P::MROWS), (unsigned)n_towers);
    hipStream_t st = (hipStream_t)stream;
    return H == 256 ? launch_fwd<256>(nbr_kind, grid, st, obs, obs_stride, self_dim, K, nbr_dim, obst_dim, B, tw, trs)
                    : launch_fwd<128>(nbr_kind, grid, st, obs, obs_stride, self_dim, K, nbr_dim, obst_dim, B, tw, trs);
}

// grid_x blocks per tower, each walking the 64-agent tiles grid_x apart
extern "C" int qs_encoder_mlp_bwd_x3(const float* obs, int32_t obs_stride, int32_t self_dim, int32_t nbr_kind, int32_t K,
                                     int32_t nbr_dim, int32_t obst_dim, int32_t B, int32_t H, const qs_enc_tower* towers,
                                     const qs_enc_train* trains, int32_t n_towers, int32_t grid_x, void* stream) {
    P::EncTowers tw{};
    P::EncTrains trs{};
    if (int rc = enc_train_args(obs, obs_stride, self_dim, nbr_kind, K, nbr_dim, obst_dim, B, H, towers, trains, n_towers,
                                true, tw, trs))
        return rc;
    if (grid_x < 1 || grid_x > (B + P::MROWS - 1) / P::MROWS) return qs_fail(QS_E_INVALID, "grid_x must be 1 .. ceil(B / 64)");
    const dim3 grid((unsigned)grid_x, (unsigned)n_towers);
    hipStream_t st = (hipStream_t)stream;
    return H == 256 ? launch_bwd<256>(nbr_kind, grid, st, K, obst_dim, B, tw, trs)
                    : launch_bwd<128>(nbr_kind, grid, st, K, obst_dim, B, tw, trs);
}
