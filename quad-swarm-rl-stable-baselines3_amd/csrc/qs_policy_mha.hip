// qs_policy_mha.hip -- the C ABI (include/quadswarm.h qs_mha_encoder_x3, qs_mha_encoder_train_x3, qs_mha_bwd_x3) over the
// multi-head attention encoder kernels (qs_policy_mha.h, qs_policy_mha_train.h).  Its own translation unit next to qs_policy_api.hip: it is built with the packed fp32 VALU
// instructions off (Makefile MHA_FLAGS) while the other policy kernels keep the code they have always compiled to.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "quadswarm.h"
#include "qs_common.h"
#include "qs_policy_mha.h"
#include "qs_policy_mha_train.h"
#include "qs_error.h"

template <int H>
static int launch_mha(dim3 grid, hipStream_t st, const float* obs, int32_t stride, int32_t so, int32_t nbw, int32_t od,
                      int32_t B, const qs::pol::MhaTowers& tw) {
    namespace P = qs::pol;
    QS_HIP_CHECK(hipFuncSetAttribute((const void*)P::mha_encoder_x3_kernel<H>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)P::mha_lds_bytes<H>()));
    hipLaunchKernelGGL(P::mha_encoder_x3_kernel<H>, grid, dim3(P::NTHR), P::mha_lds_bytes<H>(), st, obs, stride, so, nbw, od,
                       B, tw);
    QS_HIP_CHECK(hipGetLastError());
    return QS_OK;
}

// 32 agents per block, one grid row per tower
extern "C" int qs_mha_encoder_x3(const float* obs, int32_t obs_stride, int32_t self_dim, int32_t nbr_width,
                                 int32_t obst_dim, int32_t B, int32_t H, const qs_mha_tower* towers, int32_t n_towers,
                                 void* stream) {
    namespace P = qs::pol;
    if (!obs || !towers) return qs_fail(QS_E_INVALID, "NULL argument");
    if (n_towers < 1 || n_towers > QS_ATTN_MAX_TOWERS) return qs_fail(QS_E_INVALID, "n_towers must be 1 or 2");
    if (H != 128 && H != 256) return qs_fail(QS_E_INVALID, "hidden size must be 128 or 256");
    if (B < 1 || (long long)B * (obs_stride > 2 * H ? obs_stride : 2 * H) >= (1ll << 31))
        return qs_fail(QS_E_INVALID, "B >= 1, B * max(obs_stride, 2 H) below 2^31");
    if (nbr_width < 1 || nbr_width > P::MHA_NBW) return qs_fail(QS_E_INVALID, "neighbour block must be 1..64 wide");
    if (obst_dim < 1 || obst_dim > P::MHA_OBW) return qs_fail(QS_E_INVALID, "obstacle values must be 1..16");
    if (self_dim < 0 || (long long)self_dim + nbr_width + obst_dim > obs_stride)
        return qs_fail(QS_E_INVALID, "the neighbour block and the obstacle values must lie inside the obs row");
    P::MhaTowers tw{};
    for (int i = 0; i < n_towers; ++i) {
        const qs_mha_tower& t = towers[i];
        if (!(t.w_e1p && t.b_n1 && t.b_o1 && t.w_n2p && t.w_o2p && t.b_n2 && t.b_o2 && t.w_qp && t.w_kp && t.w_vp &&
              t.w_fcp && t.ln_g && t.ln_b && t.out))
            return qs_fail(QS_E_INVALID, "NULL tower pointer");
        tw.t[i] = t;
    }
    const dim3 grid((unsigned)((B + P::MHA_AG - 1) / P::MHA_AG), (unsigned)n_towers);
    hipStream_t st = (hipStream_t)stream;
    return H == 256 ? launch_mha<256>(grid, st, obs, obs_stride, self_dim, nbr_width, obst_dim, B, tw)
                    : launch_mha<128>(grid, st, obs, obs_stride, self_dim, nbr_width, obst_dim, B, tw);
}

// ---- the PPO update's forward with saves and backward (qs_policy_mha_train.h) ----
static bool mha_tower_ok(const qs_mha_tower& t) {
    return t.w_e1p && t.b_n1 && t.b_o1 && t.w_n2p && t.w_o2p && t.b_n2 && t.b_o2 && t.w_qp && t.w_kp && t.w_vp && t.w_fcp &&
           t.ln_g && t.ln_b;
}
static bool mha_saves_ok(const qs_mha_train& r) { return r.x1 && r.x && r.sm && r.xhat && r.rsig; }

template <int H>
static int launch_mha_train(dim3 grid, hipStream_t st, const float* obs, int32_t stride, int32_t so, int32_t nbw,
                            int32_t od, int32_t B, const qs::pol::MhaTowers& tw, const qs::pol::MhaTrains& tr) {
    namespace P = qs::pol;
    QS_HIP_CHECK(hipFuncSetAttribute((const void*)P::mha_encoder_train_x3_kernel<H>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)P::mha_lds_bytes<H>()));
    hipLaunchKernelGGL(P::mha_encoder_train_x3_kernel<H>, grid, dim3(P::NTHR), P::mha_lds_bytes<H>(), st, obs, stride, so,
                       nbw, od, B, tw, tr);
    QS_HIP_CHECK(hipGetLastError());
    return QS_OK;
}

extern "C" int qs_mha_encoder_train_x3(const float* obs, int32_t obs_stride, int32_t self_dim, int32_t nbr_width,
                                       int32_t obst_dim, int32_t B, int32_t H, const qs_mha_tower* towers,
                                       const qs_mha_train* trains, int32_t n_towers, void* stream) {
    namespace P = qs::pol;
    if (!obs || !towers || !trains) return qs_fail(QS_E_INVALID, "NULL argument");
    if (n_towers < 1 || n_towers > QS_ATTN_MAX_TOWERS) return qs_fail(QS_E_INVALID, "n_towers must be 1 or 2");
    if (H != 128 && H != 256) return qs_fail(QS_E_INVALID, "hidden size must be 128 or 256");
    if (B < 1 || (long long)B * (obs_stride > 2 * H ? obs_stride : 2 * H) >= (1ll << 31))
        return qs_fail(QS_E_INVALID, "B >= 1, B * max(obs_stride, 2 H) below 2^31");
    if (nbr_width < 1 || nbr_width > P::MHA_NBW) return qs_fail(QS_E_INVALID, "neighbour block must be 1..64 wide");
    if (obst_dim < 1 || obst_dim > P::MHA_OBW) return qs_fail(QS_E_INVALID, "obstacle values must be 1..16");
    if (self_dim < 0 || (long long)self_dim + nbr_width + obst_dim > obs_stride)
        return qs_fail(QS_E_INVALID, "the neighbour block and the obstacle values must lie inside the obs row");
    P::MhaTowers tw{};
    P::MhaTrains tr{};
    for (int i = 0; i < n_towers; ++i) {
        if (!(mha_tower_ok(towers[i]) && towers[i].out)) return qs_fail(QS_E_INVALID, "NULL tower pointer");
        if (!mha_saves_ok(trains[i])) return qs_fail(QS_E_INVALID, "NULL saved-activation pointer");
        tw.t[i] = towers[i];
        tr.t[i] = trains[i];
    }
    const dim3 grid((unsigned)((B + P::MHA_AG - 1) / P::MHA_AG), (unsigned)n_towers);
    hipStream_t st = (hipStream_t)stream;
    return H == 256 ? launch_mha_train<256>(grid, st, obs, obs_stride, self_dim, nbr_width, obst_dim, B, tw, tr)
                    : launch_mha_train<128>(grid, st, obs, obs_stride, self_dim, nbr_width, obst_dim, B, tw, tr);
}

template <int H>
static int launch_mha_bwd(dim3 grid, hipStream_t st, int32_t B, const qs::pol::MhaTowers& tw, const qs::pol::MhaTrains& tr) {
    namespace P = qs::pol;
    QS_HIP_CHECK(hipFuncSetAttribute((const void*)P::mha_bwd_x3_kernel<H>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)P::mha_bwd_lds_bytes<H>()));
    hipLaunchKernelGGL(P::mha_bwd_x3_kernel<H>, grid, dim3(P::NTHR), P::mha_bwd_lds_bytes<H>(), st, B, tw, tr);
    QS_HIP_CHECK(hipGetLastError());
    return QS_OK;
}

// the same 32-agent blocks; towers: the forward's packed weights (out is not used)
extern "C" int qs_mha_bwd_x3(int32_t B, int32_t H, const qs_mha_tower* towers, const qs_mha_train* trains, int32_t n_towers,
                             void* stream) {
    namespace P = qs::pol;
    static_assert(QS_MHA_NCOLMAX == 4 + 2 * P::MHA_HEADS, "colmax rows: dpre2, dpre1 per token, G_h and R_h per head");
    if (!towers || !trains) return qs_fail(QS_E_INVALID, "NULL argument");
    if (n_towers < 1 || n_towers > QS_ATTN_MAX_TOWERS) return qs_fail(QS_E_INVALID, "n_towers must be 1 or 2");
    if (H != 128 && H != 256) return qs_fail(QS_E_INVALID, "hidden size must be 128 or 256");
    if (B < 1 || (long long)B * 2 * H >= (1ll << 31)) return qs_fail(QS_E_INVALID, "B >= 1, B * 2 H below 2^31");
    P::MhaTowers tw{};
    P::MhaTrains tr{};
    for (int i = 0; i < n_towers; ++i) {
        const qs_mha_train& r = trains[i];
        if (!mha_tower_ok(towers[i])) return qs_fail(QS_E_INVALID, "NULL tower pointer");
        if (!(mha_saves_ok(r) && r.dout && r.w_fctp && r.w_qtp && r.w_ktp && r.w_vtp && r.w_n2tp && r.w_o2tp && r.gmix &&
              r.rmix && r.dpre2 && r.dpre1 && r.colmax))
            return qs_fail(QS_E_INVALID, "NULL train pointer");
        tw.t[i] = towers[i];
        tr.t[i] = r;
    }
    const dim3 grid((unsigned)((B + P::MHA_AG - 1) / P::MHA_AG), (unsigned)n_towers);
    hipStream_t st = (hipStream_t)stream;
    return H == 256 ? launch_mha_bwd<256>(grid, st, B, tw, tr) : launch_mha_bwd<128>(grid, st, B, tw, tr);
}
