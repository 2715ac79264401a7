"""The PPO update's fused MLP-family encoders (csrc/qs_policy_enc_train.h, quadswarm_amd/enc_mlp_train.py) on
test_gpu_policy_encoder's policies.  B = 1, 65, 197: one row, one row into a second tile, a ragged last tile with several
tiles per walking block; B = 197 once more with two backward blocks per tower, so that a block really walks.

Forward: the latents are bitwise the rollout kernel's (which test_gpu_policy_encoder pins to fp64).  Gradients, per tensor:
ef <= 16 et + 1e-6 with ef, et the fused path's and torch fp32 autograd's max abs error relative to max |g64|
(test_gpu_tail_train's and test_gpu_mha_train's rule).  A wrong transpose block, a missing 1 / K, a wrong (b, k) row order
or obstacle offset moves a gradient by >= 1e-2 relative.
Measured on an MI355X over the 48 cases: worst ef 1.14e-6 where its et is 4.8e-7; the trainer's flat minibatch gradient
within 5.6e-7 of the all-torch path's ("PPO update: the MLP-family encoders")."""
import copy
import functools

import pytest
import torch

from quadswarm_amd import QuadSwarmConfig, _native as NAT
from quadswarm_amd.enc_mlp_train import FusedEncoderTrain
from quadswarm_amd.env import QuadSwarmEnv
from quadswarm_amd.policy_fused import FusedRolloutPolicy
from quadswarm_amd.ppo import PolicyConfig, PPOConfig, PPOTrainer, SwarmActorCritic
from test_gpu_policy_encoder import SEED, branches, make_policy, obs_for
from test_policy_encoder_cpu import CASES

pytestmark = pytest.mark.gpu

SHAPES = pytest.mark.parametrize("case,H,B,grid_x", [(c, H, B, g) for c in CASES for H in (128, 256)
                                                     for B, g in ((1, None), (65, None), (197, None), (197, 2))])
N_GRADS = {"no_encoder": 6, "mean_embed": 10, "mlp": 12}


def latents(pol, obs):
    return pol.actor_encoder(obs), pol.critic_encoder(obs)


@functools.lru_cache(maxsize=None)
@torch.enable_grad()   # (the forward test calls it under no_grad)
def reference(case, H, B):
    """(obs, dout [2, B, 2H], fp64 gradients of sum(lat dout) for FusedEncoderTrain.params()), once per shape on the CPU."""
    pol, pol64 = make_policy(case, H)
    obs = obs_for(pol.cfg, B)
    dout = torch.randn(2, B, 2 * H, generator=torch.Generator().manual_seed(SEED + 3)) * 1e-3
    dout[:, 2::3] = 0.0        # PPO's clip: exactly zero rows (every third; row 0 keeps B = 1 a gradient)
    if B == 197:
        dout[:, :64] = 0.0     # a whole zero tile
    la, lc = latents(pol64, obs.double())
    g64 = torch.autograd.grad((la * dout[0].double()).sum() + (lc * dout[1].double()).sum(), FusedEncoderTrain(pol64).params())
    return obs, dout, g64


@SHAPES
@torch.no_grad()
def test_latents_are_the_rollout_kernels(case, H, B, grid_x):
    gpol = copy.deepcopy(make_policy(case, H)[0]).cuda()
    obs = reference(case, H, B)[0].cuda()
    la, lc = FusedEncoderTrain(gpol, grid_x).latents(obs)
    want = FusedRolloutPolicy(gpol, "x3").latents(obs)
    assert la.shape == (B, 2 * H) and torch.equal(la, want[0]) and torch.equal(lc, want[1])


@SHAPES
def test_gradients_match_fp64_autograd(case, H, B, grid_x):
    gpol = copy.deepcopy(make_policy(case, H)[0]).cuda()
    obs, dout, g64 = reference(case, H, B)
    obs, dout = obs.cuda(), dout.cuda()
    fused = FusedEncoderTrain(gpol, grid_x)
    wrt = fused.params()
    assert len(wrt) == len(g64) == 2 * (N_GRADS[CASES[case][0]] + (4 if CASES[case][4] else 0))
    loss = lambda lat: (lat[0] * dout[0]).sum() + (lat[1] * dout[1]).sum()  # noqa: E731
    gf = torch.autograd.grad(loss(fused.latents(obs)), wrt)
    assert fused.runner.grid_x == (grid_x or (B + 63) // 64)
    gt = torch.autograd.grad(loss(latents(gpol, obs)), wrt)
    worst, bad = (0.0, 0.0), []
    for i, (f, t, w) in enumerate(zip(gf, gt, g64)):
        assert f.shape == w.shape and bool(torch.isfinite(f).all()), i
        ref = w.abs().max().item()
        ef, et = ((g.double().cpu() - w).abs().max().item() / ref for g in (f, t))
        worst = max(worst, (ef, et))
        if not ef <= 16.0 * et + 1e-6:
            bad.append((i, ef, et))
    print(f"enc train grads {case} H={H} B={B} grid={grid_x}: worst ef {worst[0]:.3e} (its et {worst[1]:.3e})")
    assert not bad, bad
    with pytest.raises(RuntimeError, match="one backward per forward"):
        fused.runner.backward([dout[0], dout[1]])


@pytest.mark.parametrize("update_tail", ["x3", "torch"])
def test_trainer_update_encoder(update_tail):
    """sb_train's shape with the mlp neighbour encoder on a 16-env C3 env: an update through the kernels, the minibatch
    gradient against the all-torch path (test_trainer_update_tail's check and bound), the range fall-back."""
    cfg = QuadSwarmConfig(num_envs=16, seed=3)
    torch.manual_seed(SEED)
    pol = SwarmActorCritic(PolicyConfig.sb_train(cfg, neighbor_encoder_type="mlp")).cuda()
    env = QuadSwarmEnv(cfg)
    pcfg = PPOConfig(n_steps=8, batch_size=256, n_epochs=1)
    with pytest.raises(ValueError):
        PPOTrainer(env, pol, pcfg, update_encoder="bogus")
    with pytest.raises(ValueError):
        PPOTrainer(env, SwarmActorCritic(PolicyConfig.sb_train(cfg)).cuda(), pcfg, update_encoder="x3")
    with pytest.raises(NAT.QuadSwarmError):
        PPOTrainer(env, copy.deepcopy(pol).cpu(), pcfg, device="cpu", update_encoder="x3")
    tr = PPOTrainer(env, pol, pcfg, seed=1, update_encoder="x3", update_tail=update_tail)
    assert tr.fused_enc is not None and tr.collect_rollouts()
    stats = tr.train(max_updates=1)
    assert stats["n_updates"] == 1 and abs(stats["loss"]) < float("inf")

    st = tr.storage
    obs, act = st.flat("obs")[:256], st.flat("actions")[:256]
    adv = torch.randn(256, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))

    def grads(fused):
        lat, tail = (tr.fused_enc.latents(obs), tr.fused_tail) if fused else (None, None)
        v, lp, _ = pol.evaluate_actions(obs, act, tail=tail, lat=lat)
        loss = -(adv * torch.exp(lp - lp.detach())).mean() + 0.5 * (v.view(-1) ** 2).mean()
        gs = torch.autograd.grad(loss, list(pol.parameters()), allow_unused=True)
        return torch.cat([(a if a is not None else torch.zeros_like(p)).flatten() for a, p in zip(gs, pol.parameters())])

    flat_f, flat_t = grads(True), grads(False)
    rel = ((flat_f - flat_t).norm() / flat_t.norm()).item()
    print(f"enc minibatch (update_tail {update_tail}): |g_fused - g_torch| / |g_torch| = {rel:.2e}")
    assert rel < 1e-4
    with torch.no_grad():
        branches(pol.critic_encoder)[-1][2].weight[3, 5] = 300.0   # beyond 65504 / 256: that minibatch's encoders on torch
    with pytest.warns(UserWarning, match="split-f16 range"):
        stats = tr.train(max_updates=1)
    assert stats["n_updates"] == 1 and abs(stats["loss"]) < float("inf")
    env.close()
