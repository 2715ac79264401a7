// qs_dw_group.hip -- the C ABI (include/quadswarm.h qs_dw_group_workspace, qs_dw_group_x3) over the grouped weight-gradient
// kernel (qs_dw_group.h).  Its own translation unit, built like qs_policy_tail_train.hip with the packed fp32 VALU
// instructions off (Makefile MHA_FLAGS).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "quadswarm.h"
#include "qs_common.h"
#include "qs_dw_group.h"
#include "qs_error.h"

namespace P = qs::pol;

static int group_shape(int32_t n_jobs, int32_t H, int32_t parts) {
    if (n_jobs < 1 || n_jobs > QS_DW_GROUP_MAX_JOBS) return qs_fail(QS_E_INVALID, "n_jobs must be 1..QS_DW_GROUP_MAX_JOBS");
    if (H != 128 && H != 256) return qs_fail(QS_E_INVALID, "hidden size must be 128 or 256");
    if (parts < 1 || parts > 65535) return qs_fail(QS_E_INVALID, "parts must be 1..65535");
    return QS_OK;
}

extern "C" int qs_dw_group_workspace(int32_t n_jobs, int32_t H, int32_t parts, size_t* bytes) {
    if (!bytes) return qs_fail(QS_E_INVALID, "NULL argument");
    if (int rc = group_shape(n_jobs, H, parts)) return rc;
    *bytes = (size_t)n_jobs * parts * P::dg_slab_floats(H) * sizeof(float);
    return QS_OK;
}

static int job_check(const qs_dw_job& j, int32_t H, int32_t parts) {
    if (!j.G || !j.A || !j.colmax || !j.dW) return qs_fail(QS_E_INVALID, "NULL job pointer (G, A, colmax, dW)");
    if (j.R < 1 || j.colmax_n < 1) return qs_fail(QS_E_INVALID, "job R >= 1, colmax_n >= 1");
    if (j.ldg < H || j.ldg > 4096) return qs_fail(QS_E_INVALID, "job ldg must be H .. 4096 floats");
    long long ld = j.ldg;
    if (j.a_kind == QS_DW_A_TANH) {
        if (j.a_cols != H || j.a_rows_per != 1) return qs_fail(QS_E_INVALID, "wide job: a_cols == H, a_rows_per == 1");
        if (j.lda < H || j.lda > 4096) return qs_fail(QS_E_INVALID, "wide job lda must be H .. 4096 floats");
        if (j.lda > ld) ld = j.lda;
    } else if (j.a_kind == QS_DW_A_OBS) {
        if (j.a_cols < 1 || j.a_cols > P::DG_NC) return qs_fail(QS_E_INVALID, "narrow job a_cols must be 1..64");
        if (j.lda < 1 || j.lda > 4096 || j.a_rows_per < 1 || j.a_inner < 0)
            return qs_fail(QS_E_INVALID, "narrow job: lda 1 .. 4096, a_rows_per >= 1, a_inner >= 0");
        if ((long long)(j.a_rows_per - 1) * j.a_inner + j.a_cols > j.lda)
            return qs_fail(QS_E_INVALID, "narrow job: the gathered columns must lie inside the row of A");
        if (j.R >= (1ll << 31)) return qs_fail(QS_E_INVALID, "narrow job R must stay below 2^31");
    } else {
        return qs_fail(QS_E_INVALID, "a_kind must be a qs_dw_a_kind");
    }
    if (j.ldw < j.a_cols || j.ldw > 4096) return qs_fail(QS_E_INVALID, "job ldw must be a_cols .. 4096 floats");
    if (j.R >= (1ll << 40) || (long long)P::dg_steps_per_part((long)j.R, parts) * P::DG_STEP * ld * 4 >= (1ll << 31))
        return qs_fail(QS_E_INVALID, "rows per part x row stride too large (use more parts)");
    return QS_OK;
}

template <int H>
static int launch_group(const P::DwJobs& jobs, int32_t n_jobs, int32_t parts, float* ws, hipStream_t st) {
    QS_HIP_CHECK(hipFuncSetAttribute((const void*)P::dw_group_x3_kernel<H>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)P::dg_lds_bytes<H>()));
    hipLaunchKernelGGL(P::dw_group_x3_kernel<H>, dim3((unsigned)parts, (unsigned)n_jobs), dim3(P::dg_threads<H>()),
                       P::dg_lds_bytes<H>(), st, jobs, (int)parts, ws);
    QS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(P::dw_group_reduce_kernel<H>, dim3((unsigned)((H * H + H + 255) / 256), (unsigned)n_jobs), dim3(256),
                       0, st, jobs, (int)parts, (const float*)ws);
    QS_HIP_CHECK(hipGetLastError());
    return QS_OK;
}

extern "C" int qs_dw_group_x3(const qs_dw_job* jobs, int32_t n_jobs, int32_t H, int32_t parts, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (!jobs || !workspace) return qs_fail(QS_E_INVALID, "NULL argument");
    if (int rc = group_shape(n_jobs, H, parts)) return rc;
    if ((uintptr_t)workspace % 16) return qs_fail(QS_E_INVALID, "workspace must be 16-byte aligned");
    if (workspace_bytes < (size_t)n_jobs * parts * P::dg_slab_floats(H) * sizeof(float))
        return qs_fail(QS_E_INVALID, "workspace smaller than qs_dw_group_workspace");
    P::DwJobs tab{};
    for (int i = 0; i < n_jobs; ++i) {
        if (int rc = job_check(jobs[i], H, parts)) return rc;
        tab.j[i] = jobs[i];
    }
    return H == 256 ? launch_group<256>(tab, n_jobs, parts, (float*)workspace, (hipStream_t)stream)
                    : launch_group<128>(tab, n_jobs, parts, (float*)workspace, (hipStream_t)stream);
}
