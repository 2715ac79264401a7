// qs_policy_enc.hip -- the C ABI (include/quadswarm.h qs_encoder_mlp_x3, qs_encoder_join_x3) over the rollout policy's
// fused MLP-family encoder kernel and the attention families' join kernel (qs_policy_enc.h).  Its own translation unit, built like qs_policy_tail.hip with the packed fp32 VALU
// instructions off (Makefile MHA_FLAGS): its epilogues are float4 arithmetic the compiler would otherwise pair into
// v_pk_* forms.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "quadswarm.h"
#include "qs_common.h"
#include "qs_policy_enc.h"
#include "qs_error.h"

template <int H, int NBR>
static int launch_enc(dim3 grid, hipStream_t st, const float* obs, int32_t stride, int32_t so, int32_t K, int32_t nd,
                      int32_t od, int32_t B, const qs::pol::EncTowers& tw) {
    namespace P = qs::pol;
    QS_HIP_CHECK(hipFuncSetAttribute((const void*)P::enc_mlp_x3_kernel<H, NBR>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)P::enc_lds_bytes<H>()));
    hipLaunchKernelGGL((P::enc_mlp_x3_kernel<H, NBR>), grid, dim3(P::NTHR), P::enc_lds_bytes<H>(), st, obs, stride, so, K, nd,
                       od, B, tw);
    QS_HIP_CHECK(hipGetLastError());
    return QS_OK;
}

template <int H>
static int launch_enc_kind(int32_t kind, dim3 grid, hipStream_t st, const float* obs, int32_t stride, int32_t so, int32_t K,
                           int32_t nd, int32_t od, int32_t B, const qs::pol::EncTowers& tw) {
    switch (kind) {
        case QS_ENC_NBR_MEAN: return launch_enc<H, QS_ENC_NBR_MEAN>(grid, st, obs, stride, so, K, nd, od, B, tw);
        case QS_ENC_NBR_MLP: return launch_enc<H, QS_ENC_NBR_MLP>(grid, st, obs, stride, so, K, nd, od, B, tw);
        default: return launch_enc<H, QS_ENC_NBR_NONE>(grid, st, obs, stride, so, K, nd, od, B, tw);
    }
}

// 64 agents per block, one grid row per tower
extern "C" int qs_encoder_mlp_x3(const float* obs, int32_t obs_stride, int32_t self_dim, int32_t nbr_kind, int32_t K,
                                 int32_t nbr_dim, int32_t obst_dim, int32_t B, int32_t H, const qs_enc_tower* towers,
                                 int32_t n_towers, void* stream) {
    namespace P = qs::pol;
    if (!obs || !towers) return qs_fail(QS_E_INVALID, "NULL argument");
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
    P::EncTowers tw{};
    for (int i = 0; i < n_towers; ++i) {
        const qs_enc_tower& t = towers[i];
        bool ok = t.w_s1p && t.b_s1 && t.w_s2p && t.b_s2 && t.w_ffp && t.b_ff && t.out;
        if (nbr_kind != QS_ENC_NBR_NONE) ok = ok && t.w_n1p && t.b_n1 && t.w_n2p && t.b_n2;
        if (nbr_kind == QS_ENC_NBR_MLP) ok = ok && t.w_n3p && t.b_n3;
        if (obst_dim > 0) ok = ok && t.w_o1p && t.b_o1 && t.w_o2p && t.b_o2;
        if (!ok) return qs_fail(QS_E_INVALID, "NULL tower pointer");
        tw.t[i] = t;
    }
    const dim3 grid((unsigned)((B + P::MROWS - 1) / P::MROWS), (unsigned)n_towers);
    hipStream_t st = (hipStream_t)stream;
    return H == 256 ? launch_enc_kind<256>(nbr_kind, grid, st, obs, obs_stride, self_dim, K, nbr_dim, obst_dim, B, tw)
                    : launch_enc_kind<128>(nbr_kind, grid, st, obs, obs_stride, self_dim, K, nbr_dim, obst_dim, B, tw);
}

template <int H, int NQ>
static int launch_join(dim3 grid, hipStream_t st, const float* obs, int32_t stride, int32_t so, int32_t oo, int32_t od,
                       int32_t B, const qs::pol::JoinTowers& tw) {
    namespace P = qs::pol;
    QS_HIP_CHECK(hipFuncSetAttribute((const void*)P::enc_join_x3_kernel<H, NQ>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)P::join_lds_bytes<H>()));
    hipLaunchKernelGGL((P::enc_join_x3_kernel<H, NQ>), grid, dim3(P::NTHR), P::join_lds_bytes<H>(), st, obs, stride, so, oo, od,
                       B, tw);
    QS_HIP_CHECK(hipGetLastError());
    return QS_OK;
}

// the attention families' join: 64 agents per block, one grid row per tower
extern "C" int qs_encoder_join_x3(const float* obs, int32_t obs_stride, int32_t self_dim, int32_t obst_off, int32_t obst_dim,
                                  int32_t nbr_parts, int32_t B, int32_t H, const qs_join_tower* towers, int32_t n_towers,
                                  void* stream) {
    namespace P = qs::pol;
    if (!obs || !towers) return qs_fail(QS_E_INVALID, "NULL argument");
    if (n_towers < 1 || n_towers > QS_ATTN_MAX_TOWERS) return qs_fail(QS_E_INVALID, "n_towers must be 1 or 2");
    if (H != 128 && H != 256) return qs_fail(QS_E_INVALID, "hidden size must be 128 or 256");
    if (self_dim < 1 || self_dim > P::ENC_SW) return qs_fail(QS_E_INVALID, "self features must be 1..32");
    if (obst_dim < 0 || obst_dim > P::ENC_OBW) return qs_fail(QS_E_INVALID, "obstacle values must be 0..16");
    if (nbr_parts != 1 && nbr_parts != 2) return qs_fail(QS_E_INVALID, "nbr_parts must be 1 or 2");
    if (self_dim > obs_stride || (obst_dim > 0 && (obst_off < 0 || (long long)obst_off + obst_dim > obs_stride)))
        return qs_fail(QS_E_INVALID, "the self and obstacle values must lie inside the obs row");
    if (B < 1 || (long long)B * (obs_stride > 2 * H ? obs_stride : 2 * H) >= (1ll << 31))
        return qs_fail(QS_E_INVALID, "B >= 1, B * max(obs_stride, 2 H) below 2^31");
    P::JoinTowers tw{};
    for (int i = 0; i < n_towers; ++i) {
        const qs_join_tower& t = towers[i];
        bool ok = t.w_s1p && t.b_s1 && t.w_s2p && t.b_s2 && t.w_ffp && t.b_ff && t.nbr && t.out;
        if (obst_dim > 0) ok = ok && t.w_o1p && t.b_o1 && t.w_o2p && t.b_o2;
        if (!ok) return qs_fail(QS_E_INVALID, "NULL tower pointer");
        if (((uintptr_t)t.nbr | (uintptr_t)t.out) & 15) return qs_fail(QS_E_INVALID, "nbr and out must be 16-byte aligned");
        tw.t[i] = t;
    }
    const dim3 grid((unsigned)((B + P::MROWS - 1) / P::MROWS), (unsigned)n_towers);
    hipStream_t st = (hipStream_t)stream;
    const int32_t so = self_dim, oo = obst_dim > 0 ? obst_off : 0, od = obst_dim;
    if (H == 256)
        return nbr_parts == 2 ? launch_join<256, 2>(grid, st, obs, obs_stride, so, oo, od, B, tw)
                              : launch_join<256, 1>(grid, st, obs, obs_stride, so, oo, od, B, tw);
    return nbr_parts == 2 ? launch_join<128, 2>(grid, st, obs, obs_stride, so, oo, od, B, tw)
                          : launch_join<128, 1>(grid, st, obs, obs_stride, so, oo, od, B, tw);
}
