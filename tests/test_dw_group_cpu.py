"""Host side of the grouped weight-gradient launch (quadswarm_amd/dw_group.py, qs_dw_group_x3): the job lists plan_encoder
and plan_tail derive from a policy, and the switch's argument checks.  No device needed."""
import ctypes

import pytest
import torch

from quadswarm_amd import QuadSwarmConfig, _native as N
from quadswarm_amd.dw_group import plan_encoder, plan_tail
from quadswarm_amd.enc_mlp_train import tower_params
from quadswarm_amd.policy_fused import tail_chain
from quadswarm_amd.ppo import PolicyConfig, PPOConfig, PPOTrainer, SwarmActorCritic
from test_policy_encoder_cpu import CASES, policy_config

# per tower: 2 self + (0 | 2 mean_embed | 3 mlp) neighbour + 2 obstacle layers + 2 NP feed_forward blocks
N_JOBS = {"none": 8, "none_obst": 16, "mean": 16, "mean_obst": 24, "mlp": 18, "mlp_obst": 26}
TAILS = {"c3_default": (lambda c: PolicyConfig.for_env(c), 0), "sb_train": (lambda c: PolicyConfig.sb_train(c), 14)}


def coverage(jobs, params, H):
    """How often every element of every parameter's gradient is written by the jobs' destination blocks."""
    hits = [torch.zeros(p.shape, dtype=torch.int32) for p in params]
    for j in jobs:
        assert j.a_cols == H if j.kind == "tanh" else 1 <= j.a_cols <= 64
        hits[j.dst][j.r0:j.r0 + H, j.c0:j.c0 + j.a_cols] += 1
        if j.db is not None:
            hits[j.db][j.db_off:j.db_off + H] += 1
    return hits


@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("case", list(CASES))
def test_plan_encoder_covers_every_parameter_once(case, H):
    pol = SwarmActorCritic(policy_config(case, H))
    jobs = plan_encoder(pol)
    assert len(jobs) == N_JOBS[case] <= N.DW_GROUP_MAX_JOBS
    params = [p for enc in (pol.actor_encoder, pol.critic_encoder) for p in tower_params(enc)]
    assert all(bool((h == 1).all()) for h in coverage(jobs, params, H))
    (K, nd), gathered = (CASES[case][3], CASES[case][2]), [j for j in jobs if j.a_rows_per > 1]
    assert len(gathered) == (2 if CASES[case][0] == "mean_embed" and K > 1 else 0)
    assert all(j.rows == "BK" and (j.a_rows_per, j.a_inner, j.a_cols) == (K, nd, nd) for j in gathered)


@pytest.mark.parametrize("name", list(TAILS))
def test_plan_tail_covers_the_chain_once(name):
    make, n_jobs = TAILS[name]
    pol = SwarmActorCritic(make(QuadSwarmConfig(num_envs=4)))
    jobs = plan_tail(pol)
    assert len(jobs) == n_jobs
    params, chain = [], []
    for core, dec, head in ((pol.actor_core, pol.actor_decoder, pol.action_net), (pol.critic_core, pol.critic_decoder, pol.value_net)):
        for m in tail_chain(core, dec):
            chain += [len(params), len(params) + 1]
            params += [m.weight, m.bias]
        params += [head.weight, head.bias]
    hits = coverage(jobs, params + [pol.log_std], pol.cfg.rnn_size)
    # the chain's parameters exactly once; the heads and log_std are the backward's part sums, not jobs
    assert all(bool((h == (1 if k in chain else 0)).all()) for k, h in enumerate(hits))


def test_switch_and_abi_argument_checks():
    cfg = QuadSwarmConfig(num_envs=4)
    pol = SwarmActorCritic(PolicyConfig.sb_train(cfg, neighbor_encoder_type="mlp"))
    env = type("Env", (), dict(I=32, obs_dim=cfg.obs_dim, act_dim=4))()
    for kw in (dict(update_dw="bogus"), dict(update_dw="grouped")):   # the second: both updates on torch
        with pytest.raises(ValueError, match="update_dw"):
            PPOTrainer(env, pol, PPOConfig(n_steps=2, batch_size=8), device="cpu", gae_fn=lambda *a: None, **kw)
    L, n = N.lib(), ctypes.c_size_t()
    assert L.qs_dw_group_workspace(18, 128, 14, ctypes.byref(n)) == 0 and n.value == 18 * 14 * (128 * 128 + 128) * 4
    assert L.qs_dw_group_workspace(N.DW_GROUP_MAX_JOBS + 1, 128, 1, ctypes.byref(n)) == -1

    def call(H=128, parts=2, ws=256, ws_bytes=1 << 30, **over):
        job = dict(G=16, A=16, colmax=16, dW=16, db=None, R=100, ldg=H, lda=H, a_cols=H, a_kind=N.DW_A_TANH, a_rows_per=1,
                   a_inner=0, colmax_n=1, ldw=H)
        job.update(over)
        return L.qs_dw_group_x3((N.QsDwJob * 1)(N.QsDwJob(**job)), 1, H, parts, ws, ws_bytes, None)
    narrow = dict(a_kind=N.DW_A_OBS, a_cols=9, lda=54, ldw=9)
    for kw, msg in ((dict(H=64), b"hidden size"), (dict(parts=0), b"parts"), (dict(ws=None), b"NULL argument"),
                    (dict(ws=8), b"aligned"), (dict(ws_bytes=1000), b"workspace smaller"), (dict(G=None), b"NULL job pointer"),
                    (dict(colmax=None), b"NULL job pointer"), (dict(R=0), b"R >= 1"), (dict(ldg=4097), b"ldg"),
                    (dict(lda=64), b"lda"), (dict(a_cols=64), b"wide job"), (dict(ldw=127), b"ldw"), (dict(a_kind=2), b"a_kind"),
                    (dict(narrow, a_cols=65, ldw=65, lda=80), b"1..64"), (dict(narrow, a_cols=0), b"1..64"),
                    (dict(narrow, a_rows_per=6, a_inner=10), b"inside the row"), (dict(narrow, R=1 << 31), b"below 2^31"),
                    (dict(R=1 << 30, ldg=4096, parts=1), b"use more parts")):   # 2^30 rows x 16 KB in one part: refused
        assert call(**kw) == -1 and msg in L.qs_last_error(), (kw, L.qs_last_error())
