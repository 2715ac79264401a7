// qs_shaping.h -- the reward shaping wrapper on device (flavor B).
//
// Replaces QuadsRewardShapingWrapper (swarm_rl/env_wrappers/reward_shaping.py:19-123) as
// make_quadrotor_env_multi builds it (swarm_rl/env_wrappers/quad_utils.py:73-94): the per-agent episode sums of the
// step's reward terms (:69-76), true_reward (:78-90), the episode's action statistics (:100-106) and the per-env,
// episode-aligned annealing of the three collision coefficients (:55-61, :110-118).
//
// shaping_kernel<true> runs after every step kernel, <false> after a reset (reward_shaping.py:46-50).  It reads what
// the step wrote -- rew_info [QS_NRI, I], rew, done, the env rows -- and the action buffer the step read; the step
// and reset kernels are untouched.  One lane per drone, a 256-lane workgroup covers floor(256 / N) whole envs, so an
// env's reduction never leaves its workgroup and its result depends on the env alone (shard invariance).  The action
// sums go through LDS in drone order: a fixed summation order, no floating-point atomics (bitwise determinism).
// Everything is fp64; the stores are plain vector stores.
//
// Annealed reward: the step runs with the handle's (final) coefficients c_g; an env whose own coefficients c_e differ
// gets rew' = fl32(rew + (c_e.bin - c_g.bin) QUADCOL + (c_e.obst - c_g.obst) OBST + (c_e.sm / c_g.sm - 1) PROX): the
// QUADCOL / OBST rows are the raw -1 / 0 terms (quadrotor_multi.py:608-651) and the PROX row is linear in
// quadcol_bin_smooth_max (collisions/quadrotors.py:95-103).  An env whose c_e equals c_g keeps the step's bits.
// CPU restatement: tests/shaping_restatement.py (pinned to the reference's wrapper by tests/golden/shaping_*).
#pragma once
#include "qs_common.h"

namespace qs {

constexpr int SH_WG = 256;   // lanes per workgroup
constexpr int SH_NQ = 8;     // reduced quantities per env: sum a_k, sum a_k^2 (k < 4)

struct SBufs {
    double* acc;        // [QS_NRI, I]
    double* coef;       // [3, E]
    double* coef_used;  // [3, E]
    double* act;        // [SH_NQ, E]
    int32_t* steps;     // [E]
    double* row;        // [I, QS_NSH]
    double* tot;        // [I, QS_NSH]
    long long* tot_n;   // [I]
    double* S;          // [1]
};

struct SP {
    double anneal;      // anneal_collision_steps, 0 = off
    double dt;          // the simulation step as the reference's Python float holds it
};

__global__ void shaping_set_scalar(double* p, double v) { *p = v; }

template <bool STEP>
__global__ __launch_bounds__(SH_WG) void shaping_kernel(const KP* __restrict__ kpp, Bufs b, SBufs s, SP sp) {
    const KP& kp = *kpp;
    const int N = kp.N, E = kp.E;
    const size_t I = (size_t)kp.I;
    const int epb = SH_WG / N;                       // whole envs per workgroup (N <= QS_MAX_AGENTS = 128)
    const int t = (int)threadIdx.x;
    const int el = t / N, di = t - el * N;
    const int env = (int)blockIdx.x * epb + el;
    const bool active = el < epb && env < E;
    const size_t g = active ? (size_t)env * N + di : 0;

    if (!STEP) {   // reset(): cumulative_rewards = {}, episode_actions = [] of the selected envs; rew_coeff stays
        if (!active || (b.mask != nullptr && b.mask[env] == 0)) return;
#pragma unroll
        for (int r = 0; r < QS_NRI; ++r) s.acc[(size_t)r * I + g] = 0.0;
        if (di == 0) {
#pragma unroll
            for (int q = 0; q < SH_NQ; ++q) s.act[(size_t)q * E + env] = 0.0;
            s.steps[env] = 0;
        }
        return;
    }

    // the lanes' a_k and a_k^2; one word of padding per row: the env's summing lanes read rows q = 0..7 at the same
    // column, which would otherwise all fall into one LDS bank (row stride 2048 B)
    __shared__ double red[SH_NQ][SH_WG + 1];
    __shared__ double tots[SH_WG * SH_NQ];  // env el's totals over its drones and steps at el * SH_NQ + q
    // the handle's coefficients as the step used them (fp32, widened)
    const double cg[3] = {(double)kp.quadcol, (double)kp.prox_max, (double)kp.quadcol_obst};
    const bool anneal = sp.anneal > 0.0;
    double ce[3] = {cg[0], cg[1], cg[2]};
    double ri[QS_NRI];
    bool done = false;
    int steps = 0;
    if (active) {
        const float4 a = *reinterpret_cast<const float4*>(b.act + 4 * g);
        const double av[4] = {(double)a.x, (double)a.y, (double)a.z, (double)a.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            red[k][t] = av[k];
            red[4 + k][t] = av[k] * av[k];   // a product of two fp32 values is exact in fp64
        }
#pragma unroll
        for (int r = 0; r < QS_NRI; ++r) ri[r] = (double)b.rcomp[(size_t)r * I + g];
        done = b.done[g] != 0;
        steps = s.steps[env] + 1;
        if (anneal) {
#pragma unroll
            for (int c = 0; c < 3; ++c) ce[c] = s.coef[(size_t)c * E + env];
            if (ce[0] != cg[0] || ce[1] != cg[1] || ce[2] != cg[2]) {
                const double fsm = cg[1] != 0.0 ? ce[1] / cg[1] - 1.0 : 0.0;
                const double prox = cg[1] != 0.0 ? fsm * ri[QS_RI_PROX] : 0.0;
                b.rew[g] = (float)((double)b.rew[g] + (ce[0] - cg[0]) * ri[QS_RI_QUADCOL] +
                                   (ce[2] - cg[2]) * ri[QS_RI_OBST] + prox);
            }
        }
#pragma unroll
        for (int r = 0; r < QS_NRI; ++r) {
            ri[r] += s.acc[(size_t)r * I + g];
            s.acc[(size_t)r * I + g] = done ? 0.0 : ri[r];
        }
    }
    __syncthreads();
    // the env's first min(N, SH_NQ) lanes each sum whole quantities over the env's drones, in drone order
    if (active && di < SH_NQ) {
        for (int q = di; q < SH_NQ; q += N) {
            double v = 0.0;
            for (int j = 0; j < N; ++j) v += red[q][el * N + j];
            v += s.act[(size_t)q * E + env];
            s.act[(size_t)q * E + env] = done ? 0.0 : v;
            tots[el * SH_NQ + q] = v;
        }
    }
    __syncthreads();
    if (!active) return;
    if (di == 0) {
        s.steps[env] = done ? 0 : steps;
#pragma unroll
        for (int c = 0; c < 3; ++c) s.coef_used[(size_t)c * E + env] = ce[c];
    }
    if (!done) return;
    const double S = *s.S;
    double cn[3];   // rew_coeff for the env's next episode (:110-118): min(final * S / anneal_steps, final)
#pragma unroll
    for (int c = 0; c < 3; ++c) cn[c] = anneal ? fmin(cg[c] * S / sp.anneal, cg[c]) : cg[c];
    double row[QS_NSH];
#pragma unroll
    for (int r = 0; r < QS_NRI; ++r) row[QS_SH_SUM + r] = ri[r];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        row[QS_SH_COEF + c] = ce[c];
        row[QS_SH_ANNEAL + c] = cn[c];
    }
    row[QS_SH_S] = S;
    row[QS_SH_TRUE_REWARD] = sp.dt * -ri[QS_RI_DIST] + 1000.0 * ri[QS_RI_QUADCOL];
    const double n = (double)steps * (double)N;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double mean = tots[el * SH_NQ + k] / n;
        const double var = tots[el * SH_NQ + 4 + k] / n - mean * mean;
        row[QS_SH_ACT_MEAN + k] = mean;
        row[QS_SH_ACT_STD + k] = sqrt(fmax(var, 0.0));
    }
    row[QS_SH_LEN] = (double)steps;
    row[QS_SH_SCEN] = (kp.obst || kp.scen_b >= 0) ? (double)b.env[(size_t)QS_E_SC_MODE * E + env] : 0.0;
    row[QS_SH_REW] = sp.dt * -((double)kp.rew_pos * ri[QS_RI_DIST] + (double)kp.rew_effort * ri[QS_RI_EFFORT] +
                               (double)kp.rew_crash * ri[QS_RI_CRASH] + (double)kp.rew_orient * ri[QS_RI_ORIENT] +
                               (double)kp.rew_spin * ri[QS_RI_SPIN]) +
                     ce[0] * ri[QS_RI_QUADCOL] + (cg[1] != 0.0 ? ce[1] / cg[1] * ri[QS_RI_PROX] : 0.0) +
                     ce[2] * ri[QS_RI_OBST];
    row[QS_NSH - 1] = 0.0;
#pragma unroll
    for (int c = 0; c < QS_NSH; ++c) {
        s.row[g * QS_NSH + c] = row[c];
        s.tot[g * QS_NSH + c] += row[c];
    }
    s.tot_n[g] += 1;
    if (di == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s.coef[(size_t)c * E + env] = cn[c];
    }
}

}  // namespace qs
