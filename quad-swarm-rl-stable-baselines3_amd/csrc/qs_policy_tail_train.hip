// qs_policy_tail_train.hip -- the C ABI (include/quadswarm.h qs_policy_tail_train_x3, qs_policy_tail_bwd_x3) over the PPO
// update's tail kernels (qs_policy_tail_train.h).  Its own translation unit, built like qs_policy_tail.hip with the
// packed fp32 VALU instructions off (Makefile MHA_FLAGS); of qs_policy_train.h it takes the staging helpers only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "quadswarm.h"
#include "qs_common.h"
#define QS_TRAIN_STAGING_ONLY 1
#include "qs_policy_tail_train.h"
#include "qs_error.h"

namespace P = qs::pol;

// the checks both entry points share; fills tw / trs and the towers' largest n_out
static int tail_train_args(int64_t B, int32_t R, int32_t n_layers, const qs_tail_tower* towers, const qs_tail_train* trains,
                           int32_t n_towers, bool backward, P::TailTowers& tw, P::TailTrains& trs, int& n_out_max) {
    if (!towers || !trains) return qs_fail(QS_E_INVALID, "NULL towers / trains");
    if (n_towers < 1 || n_towers > QS_ATTN_MAX_TOWERS) return qs_fail(QS_E_INVALID, "n_towers must be 1 or 2");
    if (R != 128 && R != 256) return qs_fail(QS_E_INVALID, "R must be 128 or 256");
    if (n_layers < 0 || n_layers > QS_TAIL_MAX_LAYERS) return qs_fail(QS_E_INVALID, "n_layers must be 0..8");
    if (B < 1 || B >= (1ll << 31)) return qs_fail(QS_E_INVALID, "B must be 1 .. 2^31 - 1");
    n_out_max = 1;
    for (int i = 0; i < n_towers; ++i) {
        const qs_tail_tower& t = towers[i];
        const qs_tail_train& r = trains[i];
        if (t.n_out < 1 || t.n_out > QS_TAIL_MAX_OUT) return qs_fail(QS_E_INVALID, "n_out must be 1..8");
        bool ok = t.x && t.w_head && (t.log_std ? r.actions && r.mean : true);
        for (int l = 0; l < n_layers; ++l) ok = ok && r.y[l];
        if (backward) {
            ok = ok && r.dlat && r.head_part && (t.log_std ? r.dlogp && r.log_std_part : r.dvalues != nullptr) &&
                 (n_layers == 0 || r.colmax);
            for (int l = 0; l < n_layers; ++l) ok = ok && r.dpre[l] && r.w_chain_t[l];
        } else {
            ok = ok && t.b_head && (t.log_std ? t.log_prob != nullptr : t.out != nullptr);
            for (int l = 0; l < n_layers; ++l) ok = ok && t.w_chain[l] && t.b_chain[l];
        }
        if (!ok) return qs_fail(QS_E_INVALID, "NULL tower / train pointer");
        if (t.n_out > n_out_max) n_out_max = t.n_out;
        tw.t[i] = t;
        trs.t[i] = r;
    }
    return QS_OK;
}

template <typename K>
static int launch_tail_train(K kernel, dim3 grid, size_t lds, hipStream_t st, int64_t B, int32_t n_layers,
                             const P::TailTowers& tw, const P::TailTrains& trs) {
    QS_HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, grid, dim3(P::NTHR), lds, st, (long)B, (int)n_layers, tw, trs);
    QS_HIP_CHECK(hipGetLastError());
    return QS_OK;
}

// 64 rows per block, one grid row per tower (the rollout kernel's geometry)
extern "C" int qs_policy_tail_train_x3(int64_t B, int32_t R, int32_t n_layers, const qs_tail_tower* towers,
                                       const qs_tail_train* trains, int32_t n_towers, void* stream) {
    P::TailTowers tw{};
    P::TailTrains trs{};
    int n_out_max;
    if (int rc = tail_train_args(B, R, n_layers, towers, trains, n_towers, false, tw, trs, n_out_max)) return rc;
    const dim3 grid((unsigned)((B + P::MROWS - 1) / P::MROWS), (unsigned)n_towers);
    hipStream_t st = (hipStream_t)stream;
    return R == 256 ? launch_tail_train(P::policy_tail_train_x3_kernel<256>, grid, P::tail_lds_bytes<256>(n_layers, n_out_max),
                                        st, B, n_layers, tw, trs)
                    : launch_tail_train(P::policy_tail_train_x3_kernel<128>, grid, P::tail_lds_bytes<128>(n_layers, n_out_max),
                                        st, B, n_layers, tw, trs);
}

// grid_x blocks per tower, each walking the 64-row tiles grid_x apart
extern "C" int qs_policy_tail_bwd_x3(int64_t B, int32_t R, int32_t n_layers, const qs_tail_tower* towers,
                                     const qs_tail_train* trains, int32_t n_towers, int32_t grid_x, void* stream) {
    P::TailTowers tw{};
    P::TailTrains trs{};
    int n_out_max;
    if (int rc = tail_train_args(B, R, n_layers, towers, trains, n_towers, true, tw, trs, n_out_max)) return rc;
    if (grid_x < 1 || grid_x > (B + P::MROWS - 1) / P::MROWS)
        return qs_fail(QS_E_INVALID, "grid_x must be 1 .. ceil(B / 64)");
    const dim3 grid((unsigned)grid_x, (unsigned)n_towers);
    hipStream_t st = (hipStream_t)stream;
    return R == 256 ? launch_tail_train(P::policy_tail_bwd_x3_kernel<256>, grid, P::tail_bwd_lds_bytes<256>(n_layers, n_out_max),
                                        st, B, n_layers, tw, trs)
                    : launch_tail_train(P::policy_tail_bwd_x3_kernel<128>, grid, P::tail_bwd_lds_bytes<128>(n_layers, n_out_max),
                                        st, B, n_layers, tw, trs);
}
