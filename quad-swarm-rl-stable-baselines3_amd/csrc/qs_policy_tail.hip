// qs_policy_tail.hip -- the C ABI (include/quadswarm.h qs_policy_tail_x3) over the rollout policy's tail kernel
// (qs_policy_tail.h).  Its own translation unit, built like qs_policy_mha.hip with the packed fp32 VALU instructions
// off (Makefile MHA_FLAGS): its head and epilogue are fp32 arithmetic the compiler would otherwise pair into v_pk_* forms.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "quadswarm.h"
#include "qs_common.h"
#include "qs_policy_tail.h"
#include "qs_error.h"

template <int R>
static int launch_tail(dim3 grid, size_t lds, hipStream_t st, int64_t B, int32_t n_layers, const qs::pol::TailTowers& tw) {
    namespace P = qs::pol;
    QS_HIP_CHECK(hipFuncSetAttribute((const void*)P::policy_tail_x3_kernel<R>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
    hipLaunchKernelGGL(P::policy_tail_x3_kernel<R>, grid, dim3(P::NTHR), lds, st, (long)B, (int)n_layers, tw);
    QS_HIP_CHECK(hipGetLastError());
    return QS_OK;
}

// 64 rows per block, one grid row per tower
extern "C" int qs_policy_tail_x3(int64_t B, int32_t R, int32_t n_layers, const qs_tail_tower* towers, int32_t n_towers,
                                 void* stream) {
    namespace P = qs::pol;
    if (!towers) return qs_fail(QS_E_INVALID, "NULL towers");
    if (n_towers < 1 || n_towers > QS_ATTN_MAX_TOWERS) return qs_fail(QS_E_INVALID, "n_towers must be 1 or 2");
    if (R != 128 && R != 256) return qs_fail(QS_E_INVALID, "R must be 128 or 256");
    if (n_layers < 0 || n_layers > QS_TAIL_MAX_LAYERS) return qs_fail(QS_E_INVALID, "n_layers must be 0..8");
    if (B < 1 || B >= (1ll << 31)) return qs_fail(QS_E_INVALID, "B must be 1 .. 2^31 - 1");
    P::TailTowers tw{};
    int n_out_max = 1;
    for (int i = 0; i < n_towers; ++i) {
        const qs_tail_tower& t = towers[i];
        if (t.n_out < 1 || t.n_out > QS_TAIL_MAX_OUT) return qs_fail(QS_E_INVALID, "n_out must be 1..8");
        bool ok = t.x && t.w_head && t.b_head && t.out && (!t.log_std || t.log_prob);
        for (int l = 0; l < n_layers; ++l) ok = ok && t.w_chain[l] && t.b_chain[l];
        if (!ok) return qs_fail(QS_E_INVALID, "NULL tower pointer");
        if (t.n_out > n_out_max) n_out_max = t.n_out;
        tw.t[i] = t;
    }
    const dim3 grid((unsigned)((B + P::MROWS - 1) / P::MROWS), (unsigned)n_towers);
    hipStream_t st = (hipStream_t)stream;
    return R == 256 ? launch_tail<256>(grid, P::tail_lds_bytes<256>(n_layers, n_out_max), st, B, n_layers, tw)
                    : launch_tail<128>(grid, P::tail_lds_bytes<128>(n_layers, n_out_max), st, B, n_layers, tw);
}
