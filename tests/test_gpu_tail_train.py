"""The PPO update's fused policy tail (csrc/qs_policy_tail_train.h, quadswarm_amd/tail_train.py) against the torch
module in fp64, on test_gpu_policy_tail's policies.  B = 1, 65, 197: one row, one row into a second tile, a ragged last
tile with several tiles per block and several dW row parts; n_layers 0 (head on the 2R input), 1 (only the [R, 2R] layer
and its two-block transpose), 3 (the tile alternation and R x R transposes).

Forward: values and log_prob within max(16 e32, floor) of the fp64 module (test_gpu_policy_tail's rule and floors) and
bitwise the rollout kernel's.  Gradients, per tensor: ef <= 16 et + 1e-6 with ef, et the fused path's and torch fp32
autograd's max abs error relative to max |g64| (test_gpu_mha_train's rule).  A wrong transpose block, a missing tanh
derivative or log_std term moves a gradient by >= 1e-2 relative.
Measured on an MI355X over the 20 cases: worst err 1.2e-6 (values), 1.9e-6 (log-prob) where torch fp32's worst e32 is
1.8e-6, 7.3e-6; worst ef 4.9e-6 where its et is 4.3e-6 ("the update's tail")."""
import copy
import functools

import pytest
import torch

from quadswarm_amd.policy_fused import FusedRolloutPolicy
from quadswarm_amd.ppo import PolicyConfig, PPOConfig, PPOTrainer, SwarmActorCritic, squashed_log_prob
from quadswarm_amd.tail_train import FusedTailTrain
from test_gpu_policy_tail import SEED, floors, make_policy

pytestmark = pytest.mark.gpu

SHAPES = pytest.mark.parametrize("R,n_layers,act_dim,B", [(R, L, 4, B) for R in (128, 256) for L in (0, 1, 3)
                                                           for B in (1, 65, 197)] + [(128, 3, 2, 65), (256, 1, 2, 65)])


def tail64(pol64, la, lc, actions):
    mean = pol64.action_net(pol64.actor_decoder(pol64.actor_core(la)))
    return pol64.value_net(pol64.critic_decoder(pol64.critic_core(lc))), squashed_log_prob(mean, pol64.log_std, actions), mean


@functools.lru_cache(maxsize=None)
@torch.enable_grad()   # (the forward test calls it under no_grad)
def reference(R, n_layers, act_dim, B):
    """(latents la, lc, noise, fp64 actions, dvalues, dlogp, fp64 values, fp64 gradients of sum(values dvalues) +
    sum(log_prob dlogp) for both latents and FusedTailTrain.params()), once per shape on the CPU."""
    _, pol64 = make_policy(R, n_layers, act_dim)
    g = torch.Generator().manual_seed(SEED + 1)
    la, lc = torch.tanh(torch.randn(B, 2 * R, generator=g)), torch.tanh(torch.randn(B, 2 * R, generator=g))
    noise = (0.5 * torch.randn(B, act_dim, generator=g)).clamp(-2.5, 2.5)
    dv, dl = torch.randn(B, 1, generator=g) * 1e-3, torch.randn(B, generator=g) * 1e-3
    dl[2::3] = 0.0         # PPO's clip: exactly zero on clipped rows (every third; row 0 keeps B = 1 a gradient)
    if B == 197:
        dv[:64] = 0.0      # a whole zero tile
    la64, lc64 = la.double().requires_grad_(), lc.double().requires_grad_()
    with torch.no_grad():
        a64 = torch.tanh(tail64(pol64, la64, lc64, torch.zeros(B, act_dim).double())[2] + pol64.log_std.exp() * noise.double())
        a64 = a64.float().double()   # the stored actions are fp32: every path reads the same values
    v64, lp64, _ = tail64(pol64, la64, lc64, a64)
    g64 = torch.autograd.grad((v64 * dv.double()).sum() + (lp64 * dl.double()).sum(),
                              [la64, lc64] + FusedTailTrain(pol64).params())
    return la, lc, noise, a64, dv, dl, v64.detach(), g64


@SHAPES
@torch.no_grad()
def test_forward_matches_fp64_module_and_rollout_kernel(R, n_layers, act_dim, B):
    pol, pol64 = make_policy(R, n_layers, act_dim)
    la, lc, noise, a64, _, _, v64, _ = reference(R, n_layers, act_dim, B)
    assert a64.abs().max() < 0.9995   # the log-prob's conditioning: a condition of the inputs, not a measurement
    gpol = copy.deepcopy(pol).cuda()
    la, lc = la.cuda(), lc.cuda()
    act, rv, rlp = FusedRolloutPolicy(gpol, "x3", tail="x3").tail(la, lc, noise.cuda())
    values, lp = FusedTailTrain(gpol).evaluate(la, lc, act)
    assert values.shape == (B, 1) and lp.shape == (B,)
    assert torch.equal(values, rv) and torch.equal(lp, rlp)
    # against fp64 on the same stored actions; e32: the fp32 torch module's own deviation
    v32, lp32, _ = tail64(gpol, la, lc, act)
    want = tail64(pol64, la.double().cpu(), lc.double().cpu(), act.double().cpu())[1]
    floor, floor_lp = floors(pol, n_layers)
    for name, got, g32, w, fl in (("values", values, v32, v64, floor), ("log_prob", lp, lp32, want, floor_lp)):
        e32, err = (g32.double().cpu() - w).abs().max().item(), (got.double().cpu() - w).abs().max().item()
        print(f"tail train R={R} L={n_layers} act={act_dim} B={B} {name}: e32 {e32:.3e} err {err:.3e} "
              f"bound {max(16.0 * e32, fl):.3e}")
        assert err <= max(16.0 * e32, fl)


@SHAPES
def test_gradients_match_fp64_autograd(R, n_layers, act_dim, B):
    pol, _ = make_policy(R, n_layers, act_dim)
    la, lc, _, a64, dv, dl, _, g64 = reference(R, n_layers, act_dim, B)
    gpol = copy.deepcopy(pol).cuda()
    la, lc = la.cuda().requires_grad_(), lc.cuda().requires_grad_()
    act, dv, dl = a64.float().cuda(), dv.cuda(), dl.cuda()
    fused = FusedTailTrain(gpol)
    wrt = [la, lc] + fused.params()
    assert len(wrt) == len(g64) == 2 + 2 * (2 * n_layers + 2) + 1
    v, lp = fused.evaluate(la, lc, act)
    gf = torch.autograd.grad((v * dv).sum() + (lp * dl).sum(), wrt)
    v32, lp32, _ = tail64(gpol, la, lc, act)
    gt = torch.autograd.grad((v32 * dv).sum() + (lp32 * dl).sum(), wrt)
    worst, bad = (0.0, 0.0), []
    for i, (f, t, w) in enumerate(zip(gf, gt, g64)):
        assert f.shape == w.shape and bool(torch.isfinite(f).all()), i
        ref = w.abs().max().item()
        ef, et = ((g.double().cpu() - w).abs().max().item() / ref for g in (f, t))
        worst = max(worst, (ef, et))
        if not ef <= 16.0 * et + 1e-6:
            bad.append((i, ef, et))
    print(f"tail train grads R={R} L={n_layers} act={act_dim} B={B}: worst ef {worst[0]:.3e} (its et {worst[1]:.3e})")
    assert not bad, bad
    with pytest.raises(RuntimeError, match="one backward per forward"):
        fused.runner.backward(dv, dl)


def test_trainer_update_tail():
    """The sb_train policy shape on a 16-env C3 env: an update through the kernels, the minibatch gradient against the
    torch path (test_gpu_mha_train.test_ppo_minibatch_gradients_match_torch's check and bound), the range fall-back."""
    from quadswarm_amd import QuadSwarmConfig
    from quadswarm_amd.env import QuadSwarmEnv

    cfg = QuadSwarmConfig(num_envs=16, seed=3)
    torch.manual_seed(SEED)
    pol = SwarmActorCritic(PolicyConfig.sb_train(cfg)).cuda()
    env = QuadSwarmEnv(cfg)
    pcfg = PPOConfig(n_steps=8, batch_size=256, n_epochs=1)
    with pytest.raises(ValueError):
        PPOTrainer(env, pol, pcfg, update_tail="bogus")
    tr = PPOTrainer(env, pol, pcfg, seed=1, rollout_precision="x3", rollout_tail="x3", update_tail="x3")
    assert tr.fused_tail is not None and tr.collect_rollouts()
    stats = tr.train(max_updates=1)
    assert stats["n_updates"] == 1 and abs(stats["loss"]) < float("inf")

    st = tr.storage
    obs, act = st.flat("obs")[:256], st.flat("actions")[:256]
    adv = torch.randn(256, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))

    def grads(tail):
        v, lp, _ = pol.evaluate_actions(obs, act, tail=tail)
        loss = -(adv * torch.exp(lp - lp.detach())).mean() + 0.5 * (v.view(-1) ** 2).mean()
        gs = torch.autograd.grad(loss, list(pol.parameters()), allow_unused=True)
        return torch.cat([(a if a is not None else torch.zeros_like(p)).flatten() for a, p in zip(gs, pol.parameters())])

    flat_f, flat_t = grads(tr.fused_tail), grads(None)
    rel = ((flat_f - flat_t).norm() / flat_t.norm()).item()
    print(f"tail minibatch: |g_fused - g_torch| / |g_torch| = {rel:.2e}")
    assert rel < 1e-4
    with torch.no_grad():
        pol.actor_core[2].weight[3, 5] = 300.0   # beyond 65504 / 256: the update warns, that minibatch's tail on torch
    with pytest.warns(UserWarning, match="split-f16 range"):
        stats = tr.train(max_updates=1)
    assert stats["n_updates"] == 1 and abs(stats["loss"]) < float("inf")
    with pytest.warns(UserWarning, match="split-f16 range"):
        assert bool(torch.isfinite(grads(tr.fused_tail)).all())
    env.close()
