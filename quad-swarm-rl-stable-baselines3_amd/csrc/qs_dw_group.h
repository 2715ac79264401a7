// qs_dw_group.h -- the PPO update's weight gradients as one grouped launch per autograd node (qs_dw_group_x3).
//
// A node of the x3 update (enc_mlp_train.py, tail_train.py) ends in 8 .. 26 products dW = G^T A over the minibatch's rows:
// G a layer's pre-activation gradients [R, H], A that layer's input -- the previous layer's tanh outputs [R, H] (WIDE) or
// raw observation columns (NARROW, at most 64).  One launch walks the job table (include/quadswarm.h qs_dw_job):
//
//   grid      (part, job).  A job's R rows are ceil(R / 16) steps of 16 rows; part p takes steps [p spp, (p + 1) spp) with
//             spp = ceil(steps / parts), so a part is a whole number of steps and only the last one is ragged.  A part with
//             no rows exits before its first barrier; the reduction below skips it.
//   scales    every block forms its job's H power-of-two column scales itself from the job's colmax rows (the backward
//             kernels' per-block maxima): thread t takes column t % H and every TPC-th row, the TPC partial maxima meet in
//             LDS, and s = 2^(140 - E) from the maximum's exponent bits E, so that s m is in [2^13, 2^14) (1 for a zero or
//             non-finite maximum, the exponent clamped to [-126, 127]: encoder_train._pow2_scales' arithmetic).
//   step      as dw_x3_kernel: G's 16 x H tile (and A's, WIDE) staged TRANSPOSED as f16 hi / lo in LDS, 16 rows + 8
//             padding halves per column (48-byte stride), so a lane's MFMA operand -- 8 consecutive rows of one column --
//             is one ds_read_b128; wave w owns output rows n in [32 w, 32 w + 32) and all of A's columns, three
//             mfma_f32_32x32x16_f16 per 32 x 32 tile (hi hi, hi lo, lo hi); two steps of rows in flight in a register ring
//             ahead of the MFMAs, LDS tiles double-buffered.  G (and a WIDE A) through buffer descriptors over the part's
//             rows: a 32-bit offset per load, zeros past the part.
//   NARROW    A's columns are staged as 64 zero-padded columns (two 32 x 32 tiles per wave; the second one is skipped when
//             a_cols <= 32): thread t takes column t % 64 and XR consecutive rows of the step, row r of A at
//             A + (r / a_rows_per) lda + (r % a_rows_per) a_inner, each load bounds-checked against the part's rows and
//             a_cols.  Scale X3_SIN (raw observations), X3_SX for WIDE (tanh outputs).
//   epilogue  acc / (s_n scale_A) as float4 stores into the (job, part) slab of the workspace, [H][H] (WIDE) or [H][64],
//             followed by the part's H column sums of G (the bias gradient's part).
//   reduce    dw_group_reduce_kernel, the second launch: thread e of job j sums element e of the job's parts in part order
//             (deterministic) and writes dW[n ldw + c] or db[n]; nothing else of the destination matrix is touched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "quadswarm.h"
#include "qs_policy_x3.h"

namespace qs {
namespace pol {

constexpr int DG_STEP = 16, DG_LDR = DG_STEP + 8;   // rows per step; LDS column stride in halves (48 B)
constexpr int DG_NC = 64;                           // a NARROW job's staged columns

struct DwJobs {
    qs_dw_job j[QS_DW_GROUP_MAX_JOBS];   // by value in the kernel arguments (80 bytes each: 3200 of the 4096)
};

template <int H>
constexpr int dg_threads() { return 64 * (H / 32); }   // one wave per 32 output rows
template <int H>
constexpr size_t dg_lds_bytes() { return (size_t)2 * 4 * H * DG_LDR * 2 + (size_t)H * 4; }   // 2 x {Gh, Gl, Ah, Al}, scales
// a (job, part) slab of the workspace in floats: the part's [H][H] (or [H][64]) product, then its H column sums
constexpr size_t dg_slab_floats(int H) { return (size_t)H * H + H; }

// the rows of a job's parts: steps per part, and the parts that have rows
__host__ __device__ inline long dg_steps_per_part(long R, int parts) {
    const long steps = (R + DG_STEP - 1) / DG_STEP;
    return (steps + parts - 1) / parts;
}
__host__ __device__ inline int dg_parts_used(long R, int parts) {
    const long steps = (R + DG_STEP - 1) / DG_STEP, spp = dg_steps_per_part(R, parts);
    return (int)((steps + spp - 1) / spp);
}

// s with s m in [2^13, 2^14), an exact power of two from m's exponent bits
__device__ __forceinline__ float dg_pow2_scale(float m) {
    const int E = (int)((__float_as_uint(m) >> 23) & 0xffu);
    if (!(m > 0.f) || E == 0xff) return 1.f;
    const int k = 140 - E > 127 ? 127 : 140 - E;   // (E <= 254: k >= -114, inside the lower clamp)
    return __uint_as_float((unsigned)(k + 127) << 23);
}

template <int H, bool WIDE>
__device__ __forceinline__ void dw_group_part(const qs_dw_job& jb, int part, int parts, float* __restrict__ slab,
                                              _Float16* lds) {
    constexpr int DWT = dg_threads<H>();
    constexpr int KT = WIDE ? H / 32 : DG_NC / 32, TPC = DWT / H, RPT = DG_STEP / TPC;
    constexpr int XR = DG_STEP * DG_NC / DWT;   // NARROW: A values per thread and step, consecutive rows of one column
    constexpr int NCW = WIDE ? H : DG_NC;       // the slab's row width
    constexpr float SA = WIDE ? X3_SX : X3_SIN;
    static_assert(RPT == 8, "a thread's rows of a step leave as one 16-byte group");
    static_assert(XR == 2 || XR == 4, "narrow staging shapes");
    float* SC = reinterpret_cast<float*>(lds + (size_t)2 * 4 * H * DG_LDR);   // [H] the job's column scales
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int sc = tid % H, sr = (tid / H) * RPT;       // staging of G (and a WIDE A): column, first row of the step
    const int xc = tid % DG_NC, xr = (tid / DG_NC) * XR;   // staging of a NARROW A
    const long R = jb.R;
    const long spp = dg_steps_per_part(R, parts);
    const long r_begin = (long)part * spp * DG_STEP;
    if (r_begin >= R) return;   // (the whole block: no barrier is skipped by some threads only)
    const long r_end = r_begin + spp * DG_STEP < R ? r_begin + spp * DG_STEP : R;
    const int nrow = (int)(r_end - r_begin);
    const int steps = (nrow + DG_STEP - 1) / DG_STEP;
    const int ldg = jb.ldg, lda = jb.lda, a_cols = jb.a_cols;
    auto buf = [&](int b, int which) { return lds + ((size_t)b * 4 + which) * H * DG_LDR; };   // 0 Gh 1 Gl 2 Ah 3 Al

    // the job's column scales from its colmax rows
    {
        float m = 0.f;
        for (int q = tid / H; q < jb.colmax_n; q += TPC) m = fmaxf(m, jb.colmax[(size_t)q * H + sc]);
        float* tmp = reinterpret_cast<float*>(lds);
        tmp[tid] = m;
        __syncthreads();
        if (tid < H) {
            float v = tmp[tid];
#pragma unroll
            for (int q = 1; q < TPC; ++q) v = fmaxf(v, tmp[q * H + tid]);
            SC[tid] = dg_pow2_scale(v);
        }
        __syncthreads();
    }
    const float sg = SC[sc];

    float gv[2][RPT], av[2][WIDE ? RPT : XR];
    float csum = 0.f;   // the column's sum over the part's rows (rows in order)
    const auto rg = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(jb.G + r_begin * ldg), (short)0,
                                                      (int)((long)nrow * ldg * 4), 0x00020000);
    const auto ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(jb.A + (WIDE ? r_begin * lda : 0)), (short)0,
                                                      WIDE ? (int)((long)nrow * lda * 4) : 0, 0x00020000);
    const int voffg = (sr * ldg + sc) * 4, voffa = (sr * lda + sc) * 4;
    const unsigned rp = (unsigned)jb.a_rows_per, inner = (unsigned)jb.a_inner;
    auto load = [&](auto SL, int s) {
        constexpr int sl = decltype(SL)::value;
        const int sog = s * DG_STEP * ldg * 4;   // (a step past the part's rows reads zeros)
#pragma unroll
        for (int u = 0; u < RPT; ++u)
            gv[sl][u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rg, voffg + u * ldg * 4, sog, 0));
        if constexpr (WIDE) {
            const int soa = s * DG_STEP * lda * 4;
#pragma unroll
            for (int u = 0; u < RPT; ++u)
                av[sl][u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ra, voffa + u * lda * 4, soa, 0));
        } else {
#pragma unroll
            for (int u = 0; u < XR; ++u) {
                const long r = r_begin + (long)s * DG_STEP + xr + u;
                float v = 0.f;
                if (r < r_end && xc < a_cols) {   // inside the part's rows and the job's columns
                    const unsigned q = (unsigned)r / rp, k = (unsigned)r - q * rp;
                    v = jb.A[(size_t)q * lda + (size_t)k * inner + xc];
                }
                av[sl][u] = v;
            }
        }
    };
    auto stage = [&](auto SL, int b) {
        constexpr int sl = decltype(SL)::value;
        f16x8 gh, gl, ah, al;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            csum += gv[sl][u];
            const float g = sg * gv[sl][u];
            gh[u] = (_Float16)g;
            gl[u] = (_Float16)(g - (float)gh[u]);
            if constexpr (WIDE) {
                const float a = SA * av[sl][u];
                ah[u] = (_Float16)a;
                al[u] = (_Float16)(a - (float)ah[u]);
            }
        }
        const int off = sc * DG_LDR + sr;
        *reinterpret_cast<f16x8*>(buf(b, 0) + off) = gh;
        *reinterpret_cast<f16x8*>(buf(b, 1) + off) = gl;
        if constexpr (WIDE) {
            *reinterpret_cast<f16x8*>(buf(b, 2) + off) = ah;
            *reinterpret_cast<f16x8*>(buf(b, 3) + off) = al;
        } else {
            typedef _Float16 f16xr __attribute__((ext_vector_type(XR)));
            f16xr xh, xl;
#pragma unroll
            for (int u = 0; u < XR; ++u) {
                const float x = SA * av[sl][u];
                xh[u] = (_Float16)x;
                xl[u] = (_Float16)(x - (float)xh[u]);
            }
            *reinterpret_cast<f16xr*>(buf(b, 2) + xc * DG_LDR + xr) = xh;
            *reinterpret_cast<f16xr*>(buf(b, 3) + xc * DG_LDR + xr) = xl;
        }
    };
    f32x16 acc[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;
    const int kt = WIDE ? KT : (a_cols > 32 ? 2 : 1);   // column tiles that hold columns of A
    const int aoff = (lane & 31) * DG_LDR + (lane >> 5) * 8;
    auto mfmas = [&](int b) {
        const f16x8 gh = *reinterpret_cast<const f16x8*>(buf(b, 0) + wave * 32 * DG_LDR + aoff);
        const f16x8 gl = *reinterpret_cast<const f16x8*>(buf(b, 1) + wave * 32 * DG_LDR + aoff);
        // A's columns as the first operand, G's as the second: the result tile is [k][n], a lane holds output row
        // n = lane & 31; A's fragments stream one column tile ahead
        f16x8 ahn = *reinterpret_cast<const f16x8*>(buf(b, 2) + aoff);
        f16x8 aln = *reinterpret_cast<const f16x8*>(buf(b, 3) + aoff);
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            if (!WIDE && k >= kt) break;
            const f16x8 ah = ahn, al = aln;
            if (k + 1 < KT) {
                ahn = *reinterpret_cast<const f16x8*>(buf(b, 2) + (k + 1) * 32 * DG_LDR + aoff);
                aln = *reinterpret_cast<const f16x8*>(buf(b, 3) + (k + 1) * 32 * DG_LDR + aoff);
            }
            acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, gh, acc[k], 0, 0, 0);
            acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, gl, acc[k], 0, 0, 0);
            acc[k] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, gh, acc[k], 0, 0, 0);
        }
    };
    // step k's rows: loaded at iteration k - 2 into slot k % 2, staged at iteration k - 1 into LDS buffer k % 2,
    // multiplied at iteration k
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    load(I0{}, 0);
    load(I1{}, 1);
    stage(I0{}, 0);
    __syncthreads();
    auto iter = [&](auto SL, int s) {   // SL = s % 2
        constexpr int sl = decltype(SL)::value;
        if (s + 2 < steps) load(std::integral_constant<int, sl>{}, s + 2);   // slot s % 2 was staged last iteration
        mfmas(sl);
        if (s + 1 < steps) stage(std::integral_constant<int, sl ^ 1>{}, sl ^ 1);
        __syncthreads();
    };
    for (int s = 0; s < steps; s += 2) {
        iter(I0{}, s);
        if (s + 1 < steps) iter(I1{}, s + 1);
    }
    // the part's column sums: the TPC threads of a column through LDS (the tiles are free after the loop's barrier)
    {
        float* cs = reinterpret_cast<float*>(lds);
        cs[tid] = csum;
        __syncthreads();
        if (tid < H) {
            float v = cs[tid];
#pragma unroll
            for (int q = 1; q < TPC; ++q) v += cs[q * H + tid];
            slab[(size_t)H * H + tid] = v;
        }
    }
    // acc[k] register 4g + j: output row n = 32 wave + (lane & 31), column 32 k + 8 g + 4 (lane >> 5) + j
    const int n = wave * 32 + (lane & 31);
    const float inv = 1.f / (SC[n] * SA);
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        if (!WIDE && k >= kt) break;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int col = k * 32 + 8 * g + 4 * (lane >> 5);
            *reinterpret_cast<float4*>(slab + (size_t)n * NCW + col) =
                make_float4(acc[k][4 * g] * inv, acc[k][4 * g + 1] * inv, acc[k][4 * g + 2] * inv, acc[k][4 * g + 3] * inv);
        }
    }
}

template <int H>
__global__ __launch_bounds__(dg_threads<H>(), 1) void dw_group_x3_kernel(DwJobs jobs, int parts, float* __restrict__ ws) {
    extern __shared__ float4 smem4[];
    const qs_dw_job& jb = jobs.j[blockIdx.y];
    float* slab = ws + ((size_t)blockIdx.y * parts + blockIdx.x) * dg_slab_floats(H);
    if (jb.a_cols == H)
        dw_group_part<H, true>(jb, (int)blockIdx.x, parts, slab, reinterpret_cast<_Float16*>(smem4));
    else
        dw_group_part<H, false>(jb, (int)blockIdx.x, parts, slab, reinterpret_cast<_Float16*>(smem4));
}

// the sum over a job's parts, in part order: element e < H a_cols is dW[e / a_cols][e % a_cols], the next H are db
template <int H>
__global__ __launch_bounds__(256) void dw_group_reduce_kernel(DwJobs jobs, int parts, const float* __restrict__ ws) {
    const qs_dw_job& jb = jobs.j[blockIdx.y];
    const int a_cols = jb.a_cols, ncw = a_cols == H ? H : DG_NC, n_el = H * a_cols;
    const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (e >= n_el + H) return;
    const int used = dg_parts_used(jb.R, parts);
    const size_t slab = dg_slab_floats(H);
    const float* base = ws + (size_t)blockIdx.y * parts * slab;
    if (e < n_el) {
        const int n = e / a_cols, c = e - n * a_cols;
        const float* p = base + (size_t)n * ncw + c;
        float v = 0.f;
        for (int q = 0; q < used; ++q) v += p[q * slab];
        jb.dW[(size_t)n * jb.ldw + c] = v;
    } else if (jb.db) {
        const float* p = base + (size_t)H * H + (e - n_el);
        float v = 0.f;
        for (int q = 0; q < used; ++q) v += p[q * slab];
        jb.db[e - n_el] = v;
    }
}

}  // namespace pol
}  // namespace qs
