"""The attention families' join (csrc/qs_policy_enc.h enc_join_x3_kernel, qs_encoder_join_x3) against the fp64 module.
Latents: the neighbour rows are the fp64 module's rounded to fp32, so the kernel alone is compared; bound max(16 e32, 3e-7
(L + 1)), test_gpu_policy_encoder.py's rule with L = 3, e32 the fp32 module's deviation on the same rows; a wrong part order,
token or obstacle offset moves the latents by >= 1e-2.  Whole policy: the bounds test_gpu_policy_fused.py (2e-4) and
test_gpu_policy_mha.py (max(16 e32, 1e-5)) hold the torch join to; trainer: test_trainer_rollout_tail's log-prob rule.
Measured on an MI355X, worst err / worst e32 / smallest bound: 24 latent cases 9.6e-7 / 1.04e-6 / 6.1e-6; whole policy
1.6e-6 / 1.2e-6 / 1.3e-5; trainer log-probs 2.1e-6 / 1.05e-5 / 8.6e-4 ("the attention families' join")."""
import copy
import functools

import pytest
import torch

from quadswarm_amd import QuadSwarmConfig
from quadswarm_amd.env import QuadSwarmEnv
from quadswarm_amd.policy_fused import FusedRolloutPolicy
from quadswarm_amd.ppo import PolicyConfig, PPOConfig, PPOTrainer, SwarmActorCritic
from test_gpu_policy_encoder import SEED, TANH_ERR, obs_for   # (the seed keeps the latents' condition below: checked on the CPU)
from test_gpu_policy_mha import make_policy as make_mha_policy
from test_gpu_policy_tail import dev, floors
from test_policy_join_cpu import CASES, policy_config

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def make_policy(case, H):
    """(fp32 policy, fp64 copy) on the CPU, widened as test_gpu_policy_encoder's / test_gpu_policy_mha's (so 19, od 9)."""
    if case == "mha":
        return make_mha_policy(H, *CASES[case][1:3])
    torch.manual_seed(SEED)
    pol = SwarmActorCritic(policy_config(case, H)).eval()
    with torch.no_grad():
        for enc in (pol.actor_encoder, pol.critic_encoder):
            for m in (m for m in enc.modules() if isinstance(m, torch.nn.Linear) and m is not enc.feed_forward[0]):
                m.weight.mul_(3.0)
                m.bias.uniform_(-0.5, 0.5)
    return pol, copy.deepcopy(pol).double()


def nbr_rows(enc, obs):
    """The rows the neighbour kernels hand the join: the two tokens [B, 2H], or the pooled attention output [B, H]."""
    c, so, K = enc.cfg, enc.cfg.self_obs_dim, enc.cfg.num_use_neighbor_obs
    return enc.tokens(obs) if c.encoder_type == "attention" else enc.neighbor_encoder(
        obs[:, :so], obs[:, so:so + K * c.neighbor_obs_dim].reshape(obs.shape[0], K, -1))


@pytest.mark.parametrize("B", [1, 64, 65, 197])
@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("case", list(CASES))
@torch.no_grad()
def test_kernel_latents_match_fp64_module(case, H, B):
    pol, pol64 = make_policy(case, H)
    obs = obs_for(pol.cfg, B)
    encs64 = (pol64.actor_encoder, pol64.critic_encoder)
    want = torch.stack([enc(obs.double()) for enc in encs64])
    assert ((want.abs() > 0.05) & (want.abs() < 0.95)).double().mean() >= 0.5   # a condition of the test: off 0 and +-1
    nbr = [nbr_rows(enc, obs.double()).float().cuda().contiguous() for enc in encs64]
    gpol = copy.deepcopy(pol).cuda()
    fp = FusedRolloutPolicy(gpol, "x3", join="x3")   # (ValueError unless join_supports(gpol))
    fp.refresh()
    got = fp.join_latents(obs.cuda(), nbr)
    l32 = torch.stack([enc(obs.cuda(), n) for enc, n in zip((gpol.actor_encoder, gpol.critic_encoder), nbr)])
    e32, err = dev(l32, want), dev(got, want)
    b = max(16.0 * e32, TANH_ERR * (3 + 1))
    print(f"join latents {case} H={H} B={B}: e32 {e32:.3e} kernel {err:.3e} bound {b:.3e}")
    assert fp.packed_join is not None and got.shape == (2, B, 2 * H) and err <= b
    assert dev(fp.join_latents(obs.cuda(), nbr, critic_only=True)[1], want[1]) <= b   # n_towers = 1: predict_values' call


@pytest.mark.parametrize("tail", ["torch", "x3"])
@pytest.mark.parametrize("case", ["attn_obst", "mha"])
@torch.no_grad()
def test_fused_policy_matches_fp64_module(case, tail):
    gpol = copy.deepcopy(make_policy(case, 128)[0]).cuda()
    obs = obs_for(gpol.cfg, 65).cuda()
    fp = FusedRolloutPolicy(gpol, "x3", tail=tail, join="x3")

    def check(what, kernel):
        p64 = copy.deepcopy(gpol).double()
        a64, v64, _ = p64(obs.double(), deterministic=True)
        a32, v32, _ = gpol(obs, deterministic=True)
        a, v, _ = fp(obs, deterministic=True)
        assert (fp.packed_join is not None) == kernel and fp.packed_precision == "x3"
        e32, err = max(dev(a32, a64), dev(v32, v64)), max(dev(a, a64), dev(v, v64), dev(fp.predict_values(obs), v64))
        b = max(16.0 * e32, 1e-5) if case == "mha" else 2e-4
        print(f"join policy {case} tail={tail} {what}: e32 {e32:.3e} fused {err:.3e} bound {b:.3e}")
        assert err <= b

    check("initial", True)
    g = torch.Generator(device="cuda").manual_seed(SEED + 2)
    for p in gpol.parameters():   # an update's worth of change, in place
        p.add_(torch.randn(p.shape, device="cuda", generator=g) * 0.01)
    fp.refresh()
    check("perturbed", True)
    if case == "mha":   # sqrt(128) 30 = 339 >= 255.9: a token could leave the f16 range at the activation scale
        gpol.critic_encoder.attention_layer.layer_norm.weight[7] = 30.0
    else:
        gpol.critic_encoder.self_encoder[2].weight[3, 5] = 300.0
    with pytest.warns(UserWarning, match="x3 rollout join.*split-f16 range"):
        fp.refresh()
    check("out of range", False)


def test_trainer_collects_through_the_join_and_updates():
    """sb_train's policy on a 16-env C3 env: neighbour kernels, join and tail; test_trainer_rollout_tail's log-prob rule."""
    cfg = QuadSwarmConfig(num_envs=16, seed=3)
    torch.manual_seed(SEED)
    pol = SwarmActorCritic(PolicyConfig.sb_train(cfg)).cuda()
    env = QuadSwarmEnv(cfg)
    pcfg = PPOConfig(n_steps=8, batch_size=256, n_epochs=1)
    with pytest.raises(ValueError):   # needs rollout_precision "x3"
        PPOTrainer(env, pol, pcfg, rollout_join="x3")
    tr = PPOTrainer(env, pol, pcfg, seed=1, rollout_precision="x3", rollout_tail="x3", rollout_join="x3")
    assert tr.collect_rollouts() and tr.fused.packed_join is not None and tr.fused.packed_tail["n_layers"] == 6
    with torch.no_grad():   # per step: the attention encoder pairs rows within a batch (ppo.NeighborAttention)
        st, p64 = tr.storage, copy.deepcopy(pol).double()
        lp32 = torch.stack([pol.evaluate_actions(st.obs[t], st.actions[t])[1] for t in range(st.T)]).double()
        lp64 = torch.stack([p64.evaluate_actions(st.obs[t].double(), st.actions[t].double())[1] for t in range(st.T)])
        mean = torch.stack([p64.action_net(p64.actor_latent(st.obs[t].double())) for t in range(st.T)])
        zmax = ((torch.atanh(st.actions.double()) - mean) / p64.log_std.exp()).abs().max().item()   # the rollout's own draw
    e32, err, d32 = dev(lp32, lp64), dev(st.log_probs, lp64), dev(st.log_probs, lp32)
    b = max(16.0 * e32, floors(pol, 4 + 1 + 6)[1] * max(1.0, zmax / 2.5))
    print(f"join trainer log_prob: e32 {e32:.3e} err {err:.3e} vs fp32 module {d32:.3e} bound {b:.3e} (max |z| {zmax:.2f})")
    assert err <= b and d32 <= b
    stats = tr.train(max_updates=1)
    assert stats["n_updates"] == 1 and abs(stats["loss"]) < float("inf")
    env.close()
