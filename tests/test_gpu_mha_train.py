"""The PPO update's fused multi-head attention tokens (csrc/qs_policy_mha_train.h, quadswarm_amd/mha_train.py) against
the torch module in fp64, on test_gpu_policy_mha's policies and observations (a subset of its shapes, so tokens64's input
conditions hold and are asserted again).  B = 1, 33, 97: one agent, one agent into a second block, a ragged last block
with several dW row parts.

Gradients, per parameter tensor: ef = max |g - g64| / max |g64| of the fused path and et the same of torch fp32 autograd
on the device; required ef <= 16 et + 1e-6 (16: x3's per-product error 7e-7 against fp32's 6e-8, the forward test's
factor; the floor is test_gpu_encoder_train's).  A wrong head block, transposed operand, missing residual or
softmax-backward term moves a gradient by >= 1e-2 relative."""
import copy
import functools

import pytest
import torch

from quadswarm_amd.mha_train import FusedMhaTrain, tower_params
from quadswarm_amd.policy_fused import FusedRolloutPolicy
from test_gpu_policy_mha import bound, make_policy, obs_for, tokens64

pytestmark = pytest.mark.gpu

SHAPES = pytest.mark.parametrize("H,nd,K,B", [(H, nd, K, B) for H in (128, 256) for nd, K in ((3, 1), (16, 4))
                                             for B in (1, 33, 97)])


@functools.lru_cache(maxsize=None)
def reference(H, nd, K, B):
    """(obs, dout [2, B, 2H] at the PPO-like scale 1e-3, fp64 tokens [2, B, 2H], the 28 fp64 parameter gradients of
    sum(tokens dout)), computed once per shape on the CPU."""
    _, pol64 = make_policy(H, nd, K)
    obs = obs_for(pol64.cfg, B)
    dout = torch.randn(2, B, 2 * H, generator=torch.Generator().manual_seed(11)) * 1e-3
    params = [p for enc in (pol64.actor_encoder, pol64.critic_encoder) for p in tower_params(enc)]
    tok = tokens64(pol64, obs.double())
    g64 = torch.autograd.grad((tok * dout.double()).sum(), params)
    return obs, dout, tok.detach(), g64


@SHAPES
def test_tokens_match_fp64_module_and_rollout_kernel(H, nd, K, B):
    pol, _ = make_policy(H, nd, K)
    obs, _, want, _ = reference(H, nd, K, B)
    gpol = copy.deepcopy(pol).cuda()
    with torch.no_grad():
        got = torch.stack(FusedMhaTrain(gpol).tokens(obs.cuda()))
        t32 = torch.stack([enc.tokens(obs.cuda()) for enc in (gpol.actor_encoder, gpol.critic_encoder)])
        roll = FusedRolloutPolicy(gpol, "x3").neighbor_encodings(obs.cuda())
    e32, err = (t32.double().cpu() - want).abs().max().item(), (got.double().cpu() - want).abs().max().item()
    print(f"mha train tokens H={H} nd={nd} K={K} B={B}: e32 {e32:.3e} kernel {err:.3e} bound {bound(e32):.3e}")
    assert got.shape == (2, B, 2 * H) and err <= bound(e32)
    assert torch.equal(got, roll)


@SHAPES
def test_parameter_gradients_match_fp64_autograd(H, nd, K, B):
    pol, _ = make_policy(H, nd, K)
    obs, dout, _, g64 = reference(H, nd, K, B)
    gpol = copy.deepcopy(pol).cuda()
    obs, dout = obs.cuda(), dout.cuda()
    fused = FusedMhaTrain(gpol)
    params = fused.params()
    assert len(params) == len(g64) == 28
    gf = torch.autograd.grad((torch.stack(fused.tokens(obs)) * dout).sum(), params)
    t32 = torch.stack([enc.tokens(obs) for enc in (gpol.actor_encoder, gpol.critic_encoder)])
    gt = torch.autograd.grad((t32 * dout).sum(), params)
    worst = (0.0, 0.0)
    bad = []
    for i, (f, t, w) in enumerate(zip(gf, gt, g64)):
        ref = w.abs().max().item()
        ef, et = ((g.double().cpu() - w).abs().max().item() / ref for g in (f, t))
        worst = max(worst, (ef, et))
        if not ef <= 16.0 * et + 1e-6:
            bad.append((i, ef, et))
    print(f"mha train grads H={H} nd={nd} K={K} B={B}: worst ef {worst[0]:.3e} (its et {worst[1]:.3e})")
    assert not bad, bad
    with pytest.raises(RuntimeError, match="one backward per forward"):
        fused.runner.backward([dout[0], dout[1]])


def test_ppo_minibatch_gradients_match_torch():
    """evaluate_actions with the fused tokens (nbr=...) against the torch path, the loss and the bound of
    test_gpu_encoder_train.test_ppo_loss_gradient_bucket_matches_torch."""
    pol, _ = make_policy(256, 6, 6)
    pol = copy.deepcopy(pol).cuda()
    B = 2048
    obs = obs_for(pol.cfg, B).cuda()
    g = torch.Generator(device="cuda").manual_seed(6)
    act = torch.rand(B, pol.cfg.act_dim, device="cuda", generator=g) * 1.6 - 0.8
    adv = torch.randn(B, device="cuda", generator=g)

    def grads(nbr):
        v, lp, _ = pol.evaluate_actions(obs, act, nbr=nbr)
        loss = -(adv * torch.exp(lp - lp.detach())).mean() + 0.5 * (v.view(-1) ** 2).mean()
        gs = torch.autograd.grad(loss, list(pol.parameters()), allow_unused=True)
        return torch.cat([(a if a is not None else torch.zeros_like(p)).flatten() for a, p in zip(gs, pol.parameters())])

    flat_f, flat_t = grads(FusedMhaTrain(pol).tokens(obs)), grads(None)
    rel = ((flat_f - flat_t).norm() / flat_t.norm()).item()
    print(f"mha minibatch: |g_fused - g_torch| / |g_torch| = {rel:.2e}")
    assert rel < 1e-4


def test_trainer_updates_through_the_kernels_and_falls_back():
    from quadswarm_amd import QuadSwarmConfig
    from quadswarm_amd.env import QuadSwarmEnv
    from quadswarm_amd.ppo import PolicyConfig, PPOConfig, PPOTrainer, SwarmActorCritic

    cfg = QuadSwarmConfig.c4(num_envs=16, seed=3)
    torch.manual_seed(2)
    pol = SwarmActorCritic(PolicyConfig.for_env(cfg, encoder_type="attention")).cuda()
    env = QuadSwarmEnv(cfg)
    tr = PPOTrainer(env, pol, PPOConfig(n_steps=8, batch_size=256, n_epochs=1), seed=1, rollout_precision="x3",
                    update_precision="x3", mha_update="x3")
    assert tr.fused_mha is not None and tr.fused_update is None
    assert tr.collect_rollouts()
    w0 = pol.actor_encoder.attention_layer.fc.weight.detach().clone()
    stats = tr.train(max_updates=1)
    assert stats["n_updates"] == 1 and abs(stats["loss"]) < float("inf")
    assert not torch.equal(w0, pol.actor_encoder.attention_layer.fc.weight)
    # the context bound max_row |w_vs|_1 >= 65504 / 16: the next minibatch warns and runs on torch autograd
    at = pol.critic_encoder.attention_layer
    with torch.no_grad():
        at.w_vs.weight.mul_(4094.0 / at.w_vs.weight.abs().sum(dim=1).max().item() * 1.01)
    with pytest.warns(UserWarning, match="split-f16 range"):
        stats = tr.train(max_updates=1)
    assert stats["n_updates"] == 1 and abs(stats["loss"]) < float("inf")
    env.close()
