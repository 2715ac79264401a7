"""The rollout policy's fused tail (csrc/qs_policy_tail.h, qs_policy_tail_x3: core, decoder, heads, squashed-Gaussian
sampling and log-prob in one launch) against the torch module in fp64.

Bound per case and quantity (actions, values, log-prob): max(16 e32, floor), test_gpu_policy_mha.py's rule; e32 is the
fp32 torch module's own max abs deviation from the fp64 module on the same inputs.  floor = 3e-7 (L + 1) max(1, N1):
tanh_fast's documented absolute error (csrc/qs_policy.h) once per tanh layer on the path, L of them, plus one such term
for the input's hi / lo split (2^-22 relative, |x| <= 1), each carried to the output through the head's largest row
1-norm N1 (the layers between pass an error on with gain ~1: |tanh'| <= 1, the widened rows have 2-norm ~1).  A mean
error reaches the log-prob through d lp / d mean_d = z_d / sigma_d, |z_d| = |eps_d| <= 2.5: floor_lp = floor 2.5 sum_d
exp(-log_std_d).  The log-prob reference is squashed_log_prob(mean64, log_std64, the stored actions): what the update
recomputes, free of the atanh conditioning of a rounding difference in the action itself.  Measured on an MI355X over
the 48 kernel cases: worst err 1.3e-6 (actions), 1.2e-6 (values), 1.9e-6 (log-prob) where torch fp32's worst e32 is
1.5e-6, 1.8e-6, 2.0e-5 ("the policy tail")."""
import copy
import functools

import pytest
import torch

from quadswarm_amd import QuadSwarmConfig
from quadswarm_amd.env import QuadSwarmEnv
from quadswarm_amd.policy_fused import FusedRolloutPolicy, tail_supports
from quadswarm_amd.ppo import PolicyConfig, PPOConfig, PPOTrainer, SwarmActorCritic, squashed_log_prob

pytestmark = pytest.mark.gpu

SEED = 0    # chosen on the CPU: the fp64 reference keeps max |a| < 0.9995 at every kernel case (asserted below)
T = 64      # the kernel's row tile (csrc/qs_policy.h MROWS)
TANH_ERR = 3e-7


def widen(pol):
    """Chain weights x 3, biases +-0.5 (as test_gpu_policy_fused.make_policy), a distinct log_std per action dimension."""
    with torch.no_grad():
        for seq in (pol.actor_core, pol.actor_decoder, pol.critic_core, pol.critic_decoder):
            for m in seq:
                if isinstance(m, torch.nn.Linear):
                    m.weight.mul_(3.0)
                    m.bias.uniform_(-0.5, 0.5)
        pol.log_std.uniform_(-1.0, 0.5)
    return pol


@functools.lru_cache(maxsize=None)
def make_policy(R, n_layers, act_dim):
    torch.manual_seed(SEED)
    pc = PolicyConfig(rnn_size=R, neighbor_hidden_size=R, act_dim=act_dim, rnn_type="full" if n_layers else None,
                      rnn_num_layers=n_layers)
    pol = widen(SwarmActorCritic(pc).eval())
    return pol, copy.deepcopy(pol).double()


def floors(pol, depth):
    n1 = max(pol.action_net.weight.abs().sum(dim=1).max().item(), pol.value_net.weight.abs().sum(dim=1).max().item())
    f = TANH_ERR * (depth + 1) * max(1.0, n1)
    return f, f * 2.5 * torch.exp(-pol.log_std.detach()).sum().item()


def tail_module(pol, la, lc, noise, deterministic):
    """The torch module's tail on given latents: (mean, actions, values)."""
    mean = pol.action_net(pol.actor_decoder(pol.actor_core(la)))
    values = pol.value_net(pol.critic_decoder(pol.critic_core(lc)))
    return mean, torch.tanh(mean if deterministic else mean + noise * pol.log_std.exp()), values


def dev(x, y):
    return (x.double().cpu() - y.double().cpu()).abs().max().item()


def deviations(devs, ref64, ref32, got, ls64, ls32):
    """devs {quantity: (e32, err)} raised by: (mean, actions, values) in fp64, in fp32, the tail's three results."""
    (m64, a64, v64), (m32, a32, v32), (a, v, lp) = [[x.double().cpu() for x in t] for t in (ref64, ref32, got)]
    lp32 = squashed_log_prob(m32.float(), ls32.detach().cpu(), a32.float())
    new = {"actions": (dev(a32, a64), dev(a, a64)), "values": (dev(v32, v64), dev(v, v64)),
           "log_prob": (dev(lp32, squashed_log_prob(m64, ls64.cpu(), a32)), dev(lp, squashed_log_prob(m64, ls64.cpu(), a)))}
    return {k: tuple(max(p, q) for p, q in zip(devs.get(k, (0.0, 0.0)), new[k])) for k in new}


def judge(what, devs, floor, floor_lp):
    ok = True
    for name, (e32, err) in devs.items():
        b = max(16.0 * e32, floor_lp if name == "log_prob" else floor)
        print(f"tail {what} {name}: e32 {e32:.3e} err {err:.3e} bound {b:.3e}")
        ok = ok and err <= b
    assert ok


@pytest.mark.parametrize("B", [1, T, T + 1, 3 * T + 5])
@pytest.mark.parametrize("act_dim", [2, 4])
@pytest.mark.parametrize("n_layers", [0, 1, 3])
@pytest.mark.parametrize("R", [128, 256])
@torch.no_grad()
def test_kernel_matches_fp64_module(R, n_layers, act_dim, B):
    pol, pol64 = make_policy(R, n_layers, act_dim)
    g = torch.Generator().manual_seed(SEED + 1)
    la, lc = torch.tanh(torch.randn(B, 2 * R, generator=g)), torch.tanh(torch.randn(B, 2 * R, generator=g))
    noise = (0.5 * torch.randn(B, act_dim, generator=g)).clamp(-2.5, 2.5)   # (N(0, 1) draws alone reach |a| = 0.99999)
    gpol = copy.deepcopy(pol).cuda()
    assert tail_supports(gpol)
    fp = FusedRolloutPolicy(gpol, "x3", tail="x3")
    devs = {}
    for det in (True, False):
        ref64 = tail_module(pol64, la.double(), lc.double(), noise.double(), det)
        assert ref64[1].abs().max() < 0.9995   # the log-prob's conditioning: a condition of the test, not a measurement
        got = fp.tail(la.cuda(), lc.cuda(), noise.cuda(), deterministic=det)
        assert fp.packed_tail is not None and [tuple(x.shape) for x in got] == [(B, act_dim), (B, 1), (B,)]
        devs = deviations(devs, ref64, tail_module(gpol, la.cuda(), lc.cuda(), noise.cuda(), det), got, pol64.log_std,
                          gpol.log_std)
    judge(f"kernel R={R} L={n_layers} act={act_dim} B={B}", devs, *floors(pol, n_layers))


# tanh layers from the observations to the head, for the floor: embedding 2 + value / attention 2 + feed_forward 1 + the
# 2 core layers; multi-head attention: embed 2 through the LayerNorm's 1 / sigma <= 10 (test_gpu_policy_mha.py) + 1 + 2
FAMILIES = {"mlp": (dict(rnn_size=256), 7),
            "attention": (dict(self_obs_dim=19, neighbor_obs_dim=6, num_use_neighbor_obs=6, obstacle_obs_dim=9,
                               rnn_size=128, neighbor_hidden_size=128, encoder_type="attention"), 23)}


@pytest.mark.parametrize("family", list(FAMILIES))
@torch.no_grad()
def test_fused_policy_matches_fp64_module(family):
    kw, depth = FAMILIES[family]
    torch.manual_seed(SEED)
    gpol = widen(SwarmActorCritic(PolicyConfig(act_dim=4, rnn_type="full", rnn_num_layers=2, **kw)).eval()).cuda()
    B, pc = 33, gpol.cfg
    od = pc.self_obs_dim + pc.neighbor_obs_dim * pc.num_use_neighbor_obs + pc.obstacle_obs_dim
    obs = torch.randn(B, od, device="cuda", generator=torch.Generator(device="cuda").manual_seed(SEED + 1))
    fp, ft = FusedRolloutPolicy(gpol, "x3", tail="x3"), FusedRolloutPolicy(gpol, "x3", tail="torch")

    def module(p, x, noise, det):
        mean = p.action_net(p.actor_latent(x))
        return mean, torch.tanh(mean if det else mean + noise * p.log_std.exp()), p.predict_values(x)

    def check(what, kernel):
        p64 = copy.deepcopy(gpol).double()
        torch.manual_seed(SEED + 3)
        noise = torch.randn((B, pc.act_dim), device="cuda")   # the draw forward() makes under this seed (unclamped:
        floor, floor_lp = floors(gpol, depth)                 # the log-prob's floor takes its largest |z|)
        devs = {}
        for det in (True, False):
            ref64 = module(p64, obs.double(), noise.double(), det)
            torch.manual_seed(SEED + 3)
            got = fp(obs, deterministic=det)
            torch.manual_seed(SEED + 3)
            at = ft(obs, deterministic=det)[0]   # the torch tail under the same seed: the same noise stream
            assert (fp.packed_tail is not None) == kernel
            devs = deviations(devs, ref64, module(gpol, obs, noise, det), got, p64.log_std, gpol.log_std)
            devs["actions"] = (devs["actions"][0], max(devs["actions"][1], dev(got[0], at)))
            devs["values"] = (devs["values"][0], max(devs["values"][1], dev(fp.predict_values(obs), ref64[2])))
        judge(f"policy {family} {what}", devs, floor, floor_lp * max(1.0, noise.abs().max().item() / 2.5))

    check("initial", True)
    g = torch.Generator(device="cuda").manual_seed(SEED + 2)
    for p in gpol.parameters():   # an update's worth of change, in place
        p.add_(torch.randn(p.shape, device="cuda", generator=g) * 0.01)
    fp.refresh()
    ft.refresh()
    check("perturbed", True)
    gpol.actor_core[2].weight[3, 5] = 300.0   # beyond 65504 / 256: refresh() warns, the torch tail evaluates
    with pytest.warns(UserWarning, match="x3 rollout tail.*f16 range"):
        fp.refresh()
    check("core weight out of range", False)


def test_trainer_rollout_tail():
    """The sb_train policy shape (6 core layers of 128) on a 16-env C3 env: the log-probs the rollout stored are those
    the torch module's evaluate_actions gives for each step's batch and stored actions, and an update runs."""
    cfg = QuadSwarmConfig(num_envs=16, seed=3)
    torch.manual_seed(SEED)
    pol = SwarmActorCritic(PolicyConfig.sb_train(cfg)).cuda()
    env = QuadSwarmEnv(cfg)
    pcfg = PPOConfig(n_steps=8, batch_size=256, n_epochs=1)
    with pytest.raises(ValueError):
        PPOTrainer(env, pol, pcfg, rollout_tail="bogus")
    tr = PPOTrainer(env, pol, pcfg, seed=1, rollout_precision="x3", rollout_tail="x3")
    assert tr.collect_rollouts() and tr.fused.packed_tail is not None and tr.fused.packed_tail["n_layers"] == 6
    with torch.no_grad():   # per step: the attention encoder pairs rows within a batch (ppo.NeighborAttention), so a step's
        st, p64 = tr.storage, copy.deepcopy(pol).double()   # log-probs are those of its own batch of agents
        lp32 = torch.stack([pol.evaluate_actions(st.obs[t], st.actions[t])[1] for t in range(st.T)]).double()
        lp64 = torch.stack([p64.evaluate_actions(st.obs[t].double(), st.actions[t].double())[1] for t in range(st.T)])
        # z = (atanh(a) - mean) / sigma is the rollout's own draw here: unclamped, so the floor takes the largest |z| stored
        mean = torch.stack([p64.action_net(p64.actor_latent(st.obs[t].double())) for t in range(st.T)])
        zmax = ((torch.atanh(st.actions.double()) - mean) / p64.log_std.exp()).abs().max().item()
    e32, err, d32 = dev(lp32, lp64), dev(st.log_probs, lp64), dev(st.log_probs, lp32)
    b = max(16.0 * e32, floors(pol, 4 + 1 + 6)[1] * max(1.0, zmax / 2.5))
    print(f"tail trainer log_prob: e32 {e32:.3e} err {err:.3e} vs fp32 module {d32:.3e} bound {b:.3e} (max |z| {zmax:.2f})")
    assert err <= b and d32 <= b
    stats = tr.train(max_updates=1)
    assert stats["n_updates"] == 1 and abs(stats["loss"]) < float("inf")
    env.close()
