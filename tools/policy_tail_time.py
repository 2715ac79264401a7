#!/usr/bin/env python
"""HIP-event times and launch counts of one rollout policy evaluation with the torch tail against the fused tail
(csrc/qs_policy_tail.h, FusedRolloutPolicy(tail="x3")) on the same inputs in the same process ("the policy
tail"); with --update, of the PPO update's tail (csrc/qs_policy_tail_train.h, PPOTrainer(update_tail="x3")) against torch
autograd.

    python tools/policy_tail_time.py [--B 32768] [--iters 50] [--rounds 3] [--update [--envs 512] [--steps 8]] [--encoder]
                                     [--join]

--join: one rollout policy step of the two attention families (C3's and C4's policy shapes) with FusedRolloutPolicy(pol,
"x3", tail="x3", join="x3") (csrc/qs_policy_enc.h enc_join_x3_kernel) against join="torch", and the joined segment alone.

Two policies: C3's default (rnn_size 256, identity core, act_dim 4) and sb_train's (rnn_size 128, 6 core layers).  For
each, mha_time.py's method (per round, alternating windows of `iters` back-to-back calls between two events, after
warm-up) on the whole evaluation forward(obs) and on the tail alone (tail() on fixed latents and noise), then, in a
separate pass with the timing done, the device launches of one call of each counted with torch.profiler.

--update: the same windows on forward + backward of the tail alone (fixed latents, actions and upstream gradients at
the PPO scale 1e-3; gradients for both latents and every tail parameter) and on one whole train(max_updates=1)
minibatch of B rows on a C3 env of --envs x 8 agents and --steps steps, with update_tail "torch" and "x3".

--update --encoder: the update's MLP-family encoders (csrc/qs_policy_enc_train.h, PPOTrainer(update_encoder="x3")) at B =
4 096 and 32 768 for three shapes: the saving forward + backward + every parameter gradient of both towers' encoders alone,
torch autograd against x3, and one whole train(max_updates=1) minibatch on a synthetic rollout with update_tail "x3" and
update_encoder "torch" / "x3"; plus the backward kernel alone and the repacking alone (where the x3 time goes).

--update [--encoder] --dw grouped: the same windows also with the node's weight gradients as one grouped launch
(csrc/qs_dw_group.h, PPOTrainer(update_dw="grouped")): "*_grouped" beside "*_x3", which stays the per-product path
("calls"), launches and ms for both from the same process and rounds."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quad-swarm-rl-stable-baselines3_amd"))

import torch  # noqa: E402

from mha_time import window  # noqa: E402
from quadswarm_amd.policy_fused import FusedRolloutPolicy  # noqa: E402
from quadswarm_amd.ppo import PolicyConfig, SwarmActorCritic  # noqa: E402

POLICIES = {"c3_default": dict(act_dim=4),
            "sb_train": dict(act_dim=4, rnn_size=128, neighbor_hidden_size=128, rnn_type="full", rnn_num_layers=6)}


def launches(fn):
    """Device kernels one call of fn enqueues."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)


def measure(fns, a, **info):
    """Warm-up, then per round one window of every function in turn; launch counts afterwards.  One JSON line."""
    for _ in range(5):
        for f in fns.values():
            f()
    ms = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, f in fns.items():
            ms[k].append(window(f, a.iters))
    n = {k: launches(f) for k, f in fns.items()}
    best = {k: min(v) for k, v in ms.items()}
    print(json.dumps(dict(ms=ms, launches=n, **info, **{k[:-3] + "_speedup": best[k[:-3] + "_torch"] / best[k]
                                                         for k in fns if k.endswith("_x3")})))


def update_mode(a):
    from quadswarm_amd import QuadSwarmConfig
    from quadswarm_amd.env import QuadSwarmEnv
    from quadswarm_amd.ppo import PPOConfig, PPOTrainer
    from quadswarm_amd.tail_train import FusedTailTrain, torch_tail

    cfg = QuadSwarmConfig(num_envs=a.envs, seed=3)
    env = QuadSwarmEnv(cfg)
    for name, make in (("c3_default", PolicyConfig.for_env), ("sb_train", PolicyConfig.sb_train)):
        torch.manual_seed(0)
        pol = SwarmActorCritic(make(cfg)).cuda()
        pc, B = pol.cfg, a.B
        lat = torch.tanh(torch.randn(2, B, 2 * pc.rnn_size, device="cuda")).requires_grad_()
        act = torch.rand(B, pc.act_dim, device="cuda") * 1.6 - 0.8
        dv, dl = torch.randn(B, 1, device="cuda") * 1e-3, torch.randn(B, device="cuda") * 1e-3
        fused = FusedTailTrain(pol)
        wrt = [lat] + fused.params()

        def fwd_bwd(tail):
            v, lp = tail(lat[0], lat[1], act)
            return torch.autograd.grad((v * dv).sum() + (lp * dl).sum(), wrt)

        fns = {"tail_torch": lambda: fwd_bwd(lambda *x: torch_tail(pol, *x)), "tail_x3": lambda: fwd_bwd(fused)}
        if a.dw == "grouped":
            grouped = FusedTailTrain(pol, dw="grouped")
            fns["tail_grouped"] = lambda: fwd_bwd(grouped)
        ref = fns["tail_torch"]()
        diff = max(((x - y).abs().max() / y.abs().max()).item() for x, y in zip(fns["tail_x3"](), ref))
        for mode in ("torch", "x3"):
            tr = PPOTrainer(env, pol, PPOConfig(n_steps=a.steps, batch_size=B, n_epochs=1), seed=1, rollout_precision="x3",
                            update_tail=mode)
            assert tr.collect_rollouts() and tr.storage.T * tr.storage.I >= B
            fns["minibatch_" + mode] = lambda tr=tr: tr.train(max_updates=1)
        if a.dw == "grouped":
            tr = PPOTrainer(env, pol, PPOConfig(n_steps=a.steps, batch_size=B, n_epochs=1), seed=1, rollout_precision="x3",
                            update_tail="x3", update_dw="grouped")
            assert tr.collect_rollouts()
            fns["minibatch_grouped"] = lambda tr=tr: tr.train(max_updates=1)
        measure(fns, a, policy=name, B=B, R=pc.rnn_size, n_layers=len(fused.runner.chains[0]),
                max_rel_grad_diff_tail_vs_torch_fp32=diff)
    env.close()


# --encoder: the MLP-family policies (csrc/qs_policy_enc.h): sb_train's shape with the mlp neighbour encoder, and the
# obstacle baseline's (no_encoder over 2 skipped pos_vel neighbours, 9 obstacle values, rnn_size 256)
ENC_POLICIES = {"sb_train_mlp": dict(self_obs_dim=18, neighbor_obs_dim=6, num_use_neighbor_obs=6, act_dim=4, rnn_size=128,
                                     neighbor_hidden_size=128, rnn_type="full", rnn_num_layers=6,
                                     neighbor_encoder_type="mlp"),
                "obst_no_encoder": dict(self_obs_dim=19, neighbor_obs_dim=6, num_use_neighbor_obs=2, obstacle_obs_dim=9,
                                        act_dim=4, neighbor_encoder_type="no_encoder")}


def encoder_mode(a):
    """One rollout policy step: the torch module (what the rollout runs with rollout_encoder "torch") against
    FusedRolloutPolicy(pol, "x3", tail="x3") (qs_encoder_mlp_x3 + qs_policy_tail_x3), and the encoder launch alone."""
    for name, kw in ENC_POLICIES.items():
        torch.manual_seed(0)
        pc = PolicyConfig(**kw)
        pol = SwarmActorCritic(pc).cuda().eval()
        obs = torch.randn(a.B, pc.self_obs_dim + pc.neighbor_obs_dim * pc.num_use_neighbor_obs + pc.obstacle_obs_dim,
                          device="cuda")
        fp = FusedRolloutPolicy(pol, "x3", tail="x3")
        fp.refresh()
        assert fp.packed_precision == "x3" and fp.packed_tail is not None
        with torch.no_grad():
            fns = {"step_torch": lambda: pol(obs), "step_x3": lambda: fp(obs), "encoder_x3": lambda: fp.latents(obs),
                   "encoder_torch": lambda: (pol.actor_encoder(obs), pol.critic_encoder(obs))}
            diff = max((x - y).abs().max().item() for x, y in zip(fns["encoder_x3"](), fns["encoder_torch"]()))
            measure(fns, a, policy=name, B=a.B, R=pc.rnn_size, max_abs_diff_latents_vs_torch_fp32=diff)


# --join: the attention families (csrc/qs_policy_enc.h enc_join_x3_kernel) at the C3 shape (the attention neighbour encoder)
# and the C4 shape (the multi-head attention encoder), rnn_size 256, identity core
JOIN_POLICIES = {"c3_attention": dict(self_obs_dim=18, neighbor_obs_dim=6, num_use_neighbor_obs=6, act_dim=4),
                 "c4_mha": dict(self_obs_dim=19, neighbor_obs_dim=6, num_use_neighbor_obs=2, obstacle_obs_dim=9, act_dim=4,
                                encoder_type="attention")}


def join_mode(a):
    """One rollout policy step of FusedRolloutPolicy(pol, "x3", tail="x3") with join "torch" against join "x3" (neighbour
    kernels + qs_encoder_join_x3 + qs_policy_tail_x3), and the segment alone on fixed neighbour rows: the torch join's
    launches against the one join launch."""
    for name, kw in JOIN_POLICIES.items():
        torch.manual_seed(0)
        pc = PolicyConfig(**kw)
        pol = SwarmActorCritic(pc).cuda().eval()
        obs = torch.randn(a.B, pc.self_obs_dim + pc.neighbor_obs_dim * pc.num_use_neighbor_obs + pc.obstacle_obs_dim,
                          device="cuda")
        fps = {mode: FusedRolloutPolicy(pol, "x3", tail="x3", join=mode) for mode in ("torch", "x3")}
        for fp in fps.values():
            fp.refresh()
            assert fp.packed_precision == "x3" and fp.packed_tail is not None
        ft, fx = fps["torch"], fps["x3"]
        assert fx.packed_join is not None
        with torch.no_grad():
            nbr = fx.neighbor_encodings(obs).clone()
            fns = {"step_torch": lambda: ft(obs), "step_x3": lambda: fx(obs),
                   "join_torch": lambda: [ft._encode(enc, obs, nbr[i], ft.packed[i]) for i, enc in enumerate(ft.encs)],
                   "join_x3": lambda: fx.join_latents(obs, nbr)}
            diff = max((x - y).abs().max().item() for x, y in zip(fns["join_x3"](), fns["join_torch"]()))
            measure(fns, a, policy=name, B=a.B, R=pc.rnn_size, max_abs_diff_latents_vs_torch_join=diff)


ENC_POLICIES_UPDATE = dict(ENC_POLICIES, c3_mean_embed=dict(self_obs_dim=18, neighbor_obs_dim=6, num_use_neighbor_obs=6,
                                                            act_dim=4, neighbor_encoder_type="mean_embed"))


def update_encoder_mode(a):
    from types import SimpleNamespace

    from quadswarm_amd import _native as NAT
    from quadswarm_amd.enc_mlp_train import FusedEncoderTrain
    from quadswarm_amd.ppo import PPOConfig, PPOTrainer

    for name, kw in ENC_POLICIES_UPDATE.items():
        for B in (4096, 32768):
            torch.manual_seed(0)
            pc = PolicyConfig(**kw)
            pol = SwarmActorCritic(pc).cuda()
            od = pc.self_obs_dim + pc.neighbor_obs_dim * pc.num_use_neighbor_obs + pc.obstacle_obs_dim
            obs = torch.randn(B, od, device="cuda")
            dout = torch.randn(2, B, 2 * pc.rnn_size, device="cuda") * 1e-3
            fused = FusedEncoderTrain(pol)
            wrt = fused.params()

            def fwd_bwd(lat):
                la, lc = lat(obs)
                return torch.autograd.grad((la * dout[0]).sum() + (lc * dout[1]).sum(), wrt)

            fns = {"encoders_torch": lambda: fwd_bwd(lambda o: (pol.actor_encoder(o), pol.critic_encoder(o))),
                   "encoders_x3": lambda: fwd_bwd(fused.latents)}
            if a.dw == "grouped":
                grouped = FusedEncoderTrain(pol, dw="grouped")
                fns["encoders_grouped"] = lambda: fwd_bwd(grouped.latents)
            ref = fns["encoders_torch"]()
            diff = max(((x - y).abs().max() / y.abs().max()).item() for x, y in zip(fns["encoders_x3"](), ref))
            # a synthetic rollout of one minibatch: the trainer reads nothing of the env but its sizes
            env = SimpleNamespace(I=B, obs_dim=od, act_dim=pc.act_dim)
            for mode in ("torch", "x3") + (("grouped",) if a.dw == "grouped" else ()):
                tr = PPOTrainer(env, pol, PPOConfig(n_steps=1, batch_size=B, n_epochs=1, learning_rate=0.0), seed=1,
                                fused_rollout=False, update_tail="x3", update_encoder="torch" if mode == "torch" else "x3",
                                update_dw="grouped" if mode == "grouped" else "calls")
                st = tr.storage
                with torch.no_grad():
                    st.obs[0].copy_(obs)
                    act, val, lp = pol(obs)
                    st.actions[0].copy_(act)
                    st.values[0].copy_(val.view(-1))
                    st.log_probs[0].copy_(lp)
                    st.advantages[0].normal_()
                    st.returns[0].normal_()
                fns["minibatch_" + mode] = lambda tr=tr: tr.train(max_updates=1)
            # where the x3 time goes: the backward kernel alone (on the buffers the last backward left) and the repacking
            r = fused.runner
            kept = fused.latents(obs)   # (held: the kernel reads the forward's outputs)

            def bwd_only():
                for i in range(2):
                    r.towers[i].out, r.trains[i].dout = kept[i].data_ptr(), dout[i].data_ptr()
                NAT.check(r.L.qs_encoder_mlp_bwd_x3(*r._args(obs), r.grid_x, r._stream(obs.device)), "qs_encoder_mlp_bwd_x3")

            fns["bwd_kernel_only"] = bwd_only
            fns["pack_only"] = r._pack
            measure(fns, a, policy=name, B=B, H=pc.rnn_size, grid_x=r.grid_x, max_rel_grad_diff_x3_vs_torch_fp32=diff)


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("B", 32768), ("iters", 50), ("rounds", 3), ("envs", 512), ("steps", 8)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--update", action="store_true")
    ap.add_argument("--encoder", action="store_true")
    ap.add_argument("--dw", choices=("calls", "grouped"), default="calls")
    ap.add_argument("--join", action="store_true")
    a = ap.parse_args()
    if a.join:
        return join_mode(a)
    if a.encoder and a.update:
        return update_encoder_mode(a)
    if a.encoder:
        return encoder_mode(a)
    if a.update:
        return update_mode(a)
    for name, kw in POLICIES.items():
        torch.manual_seed(0)
        pc = PolicyConfig(**kw)
        pol = SwarmActorCritic(pc).cuda().eval()
        B, R = a.B, pc.rnn_size
        obs = torch.randn(B, pc.self_obs_dim + pc.neighbor_obs_dim * pc.num_use_neighbor_obs, device="cuda")
        lat = torch.tanh(torch.randn(2, B, 2 * R, device="cuda"))
        noise = torch.randn(B, pc.act_dim, device="cuda")
        fns = {}
        for mode in ("torch", "x3"):
            fp = FusedRolloutPolicy(pol, "x3", tail=mode)
            fp.refresh()
            assert mode == "torch" or fp.packed_tail is not None
            fns["forward_" + mode] = lambda fp=fp: fp(obs)
            fns["tail_" + mode] = lambda fp=fp: fp.tail(lat[0], lat[1], noise)
        diff = max((x - y).abs().max().item() for x, y in zip(fns["tail_x3"](), fns["tail_torch"]()))
        measure(fns, a, policy=name, B=B, R=R, n_layers=pc.rnn_num_layers if pc.rnn_type == "full" else 0,
                max_abs_diff_tail_vs_torch_fp32=diff)


if __name__ == "__main__":
    main()
