"""The grouped weight-gradient kernel (csrc/qs_dw_group.h, qs_dw_group_x3) against fp64, alone and under the update's
autograd nodes and the trainer.  R = 1, 17, 300 rows with 1 and 3 parts: one row, a ragged second 16-row step, several steps
per part with a ragged last part.

Per tensor ef <= 16 et + 1e-6 with ef, et the kernel's and a plain torch fp32 product's max abs error relative to max |fp64|
(test_gpu_enc_mlp_train's rule).  A wrong block corner, part boundary, gather stride or column scale moves a result by >= 1e-2.
Measured on an MI355X: worst ef 9.8e-7 (kernel; its et 4.4e-7), 1.14e-6 (encoder nodes; et 4.8e-7), 4.88e-6 (tail nodes; et
4.34e-6); the trainer's flat minibatch gradient within 5.3e-7 of the all-torch path's ("the grouped
weight-gradient kernel")."""
import copy
import ctypes

import pytest
import torch

import test_gpu_enc_mlp_train as ENC
import test_gpu_tail_train as TAIL
from quadswarm_amd import QuadSwarmConfig, _native as NAT
from quadswarm_amd.enc_mlp_train import FusedEncoderTrain
from quadswarm_amd.env import QuadSwarmEnv
from quadswarm_amd.ppo import PolicyConfig, PPOConfig, PPOTrainer, SwarmActorCritic
from quadswarm_amd.tail_train import FusedTailTrain
from test_policy_encoder_cpu import CASES

pytestmark = pytest.mark.gpu


def judge(what, got, t32, w64):
    """[(ef, et)] per tensor under the rule; prints the worst."""
    pairs = []
    for f, t, w in zip(got, t32, w64):
        assert f.shape == w.shape and bool(torch.isfinite(f).all())
        ref = w.abs().max().item()
        pairs.append(tuple((g.double().cpu() - w).abs().max().item() / ref for g in (f, t)))
    worst = max(pairs)
    print(f"dw group {what}: worst ef {worst[0]:.3e} (its et {worst[1]:.3e})")
    assert not [(i, p) for i, p in enumerate(pairs) if not p[0] <= 16.0 * p[1] + 1e-6], pairs


@pytest.mark.parametrize("H,R,parts", [(H, R, p) for H in (128, 256) for R in (1, 17, 300) for p in (1, 3)])
def test_kernel_matches_fp64(H, R, parts):
    g = torch.Generator().manual_seed(7 + R)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    # G [R, 2H]: column magnitudes over 1e-9 .. 1e-2, one all-zero column per half, every third row zero (row 0 kept)
    G = rnd(R, 2 * H) * 10.0 ** (-9.0 + 7.0 * torch.rand(2 * H, generator=g))
    G[:, [5, H + 5]] = 0.0
    G[2::3] = 0.0
    A = torch.tanh(rnd(R, H))
    obs = (rnd(R, 70) * 20.0).clamp(-50.0, 50.0)          # narrow rows; the gathered job: 6 rows of G per row of obs
    G6 = rnd(6 * R, H) * 10.0 ** (-9.0 + 7.0 * torch.rand(H, generator=g))
    G6[:, 5] = 0.0
    G6[2::3] = 0.0
    big0 = rnd(H + 7, 2 * H + 12)                         # the interior block's matrix: rows 3 .., columns 8 .. stay
    d = lambda x: x.cuda().contiguous()  # noqa: E731
    Gd, Ad, obsd, G6d, big = d(G), d(A), d(obs), d(G6), d(big0)
    Gc = Gd[:, :H].contiguous()

    def colmax(x, n):   # the true maxima split over n row ranges
        return torch.stack([c.abs().amax(0) if c.numel() else torch.zeros(x.shape[1]) for c in x.tensor_split(n)]).cuda()

    cm = {"g0": colmax(G[:, :H], 1), "g1": colmax(G[:, H:], 3), "g6": colmax(G6, 3)}
    outs, jobs = [], (NAT.QsDwJob * 7)()

    def job(i, Gt, ldg, At, lda, cols, kind, cmax, dW, ldw, db=None, per=1, inner=0):
        q = jobs[i]
        q.G, q.ldg, q.A, q.lda, q.a_cols, q.a_kind, q.a_rows_per, q.a_inner = Gt, ldg, At, lda, cols, kind, per, inner
        q.R, q.colmax, q.colmax_n, q.dW, q.ldw, q.db = R * per, cmax.data_ptr(), cmax.shape[0], dW, ldw, db

    def fresh(*s):
        outs.append(torch.full(s, 7.0, device="cuda"))
        return outs[-1]

    W0, b0 = fresh(H, H), fresh(H)
    job(0, Gc.data_ptr(), H, Ad.data_ptr(), H, H, NAT.DW_A_TANH, cm["g0"], W0.data_ptr(), H, b0.data_ptr())
    job(1, Gd.data_ptr() + 4 * H, 2 * H, Ad.data_ptr(), H, H, NAT.DW_A_TANH, cm["g1"],
        big.data_ptr() + 4 * (3 * big.shape[1] + 8), big.shape[1])
    want = [G[:, :H].double().t() @ A.double(), G[:, :H].double().sum(0)]
    t32 = [Gc.t() @ Ad, Gc.sum(0)]
    for i, (off, cols) in enumerate(((0, 9), (9, 18), (27, 36), (6, 64))):
        Wn = fresh(H, cols)
        job(2 + i, Gc.data_ptr(), H, obsd.data_ptr() + 4 * off, 70, cols, NAT.DW_A_OBS, cm["g0"], Wn.data_ptr(), cols)
        want.append(G[:, :H].double().t() @ obs[:, off:off + cols].double())
        t32.append(Gc.t() @ obsd[:, off:off + cols])
    W6, b6 = fresh(H, 6), fresh(H)   # row r of G6 against obs[r // 6, 4 + 6 (r % 6) ..][:6]
    job(6, G6d.data_ptr(), H, obsd.data_ptr() + 4 * 4, 70, 6, NAT.DW_A_OBS, cm["g6"], W6.data_ptr(), 6, b6.data_ptr(), 6, 6)
    X6 = obs[:, 4:40].reshape(6 * R, 6)
    want += [G6.double().t() @ X6.double(), G6.double().sum(0)]
    t32 += [G6d.t() @ d(X6), G6d.sum(0)]
    want.insert(2, G[:, H:].double().t() @ A.double())
    t32.insert(2, Gd[:, H:].t() @ Ad)

    L, n = NAT.lib(), ctypes.c_size_t(7 * parts * (H * H + H) * 4)   # qs_dw_group_workspace's (test_dw_group_cpu)
    ws = torch.empty(n.value // 4, device="cuda")
    NAT.check(L.qs_dw_group_x3(jobs, 7, H, parts, ctypes.c_void_p(ws.data_ptr()), n.value,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "qs_dw_group_x3")
    torch.cuda.synchronize()
    got = [W0, b0, big[3:3 + H, 8:8 + H]] + outs[2:]
    judge(f"kernel H={H} R={R} parts={parts}", got, t32, want)
    big0[3:3 + H, 8:8 + H] = big[3:3 + H, 8:8 + H].cpu()
    assert torch.equal(big.cpu(), big0)                                  # around the interior block: bitwise unchanged
    for W, b in ((W0, b0), (big[3:3 + H, 8:8 + H], None), (W6, b6)):     # the zero column: exactly zero
        assert not W[5].any() and (b is None or b[5] == 0)


@pytest.mark.parametrize("case,H,B", [(c, H, B) for c in CASES for H in (128, 256) for B in (1, 65, 197)])
def test_encoder_node_gradients(case, H, B):
    gpol = copy.deepcopy(ENC.make_policy(case, H)[0]).cuda()
    obs, dout, g64 = ENC.reference(case, H, B)
    obs, dout = obs.cuda(), dout.cuda()
    fused = FusedEncoderTrain(gpol, dw="grouped")
    wrt, loss = fused.params(), lambda lat: (lat[0] * dout[0]).sum() + (lat[1] * dout[1]).sum()
    gf = torch.autograd.grad(loss(fused.latents(obs)), wrt)
    gt = torch.autograd.grad(loss(ENC.latents(gpol, obs)), wrt)
    judge(f"encoder node {case} H={H} B={B}", gf, gt, g64)


@pytest.mark.parametrize("R,n_layers,B", [(R, L, B) for R in (128, 256) for L in (0, 1, 3) for B in (1, 65, 197)])
def test_tail_node_gradients(R, n_layers, B):
    la, lc, _, a64, dv, dl, _, g64 = TAIL.reference(R, n_layers, 4, B)
    gpol = copy.deepcopy(TAIL.make_policy(R, n_layers, 4)[0]).cuda()
    la, lc = la.cuda().requires_grad_(), lc.cuda().requires_grad_()
    act, dv, dl = a64.float().cuda(), dv.cuda(), dl.cuda()
    fused = FusedTailTrain(gpol, dw="grouped")
    wrt = [la, lc] + fused.params()
    v, lp = fused.evaluate(la, lc, act)
    gf = torch.autograd.grad((v * dv).sum() + (lp * dl).sum(), wrt)
    v32, lp32, _ = TAIL.tail64(gpol, la, lc, act)
    gt = torch.autograd.grad((v32 * dv).sum() + (lp32 * dl).sum(), wrt)
    judge(f"tail node R={R} L={n_layers} B={B}", gf, gt, g64)


def test_trainer_update_dw_grouped():
    """test_trainer_update_encoder's env, policy, check and bound with both x3 updates on the grouped launch."""
    cfg = QuadSwarmConfig(num_envs=16, seed=3)
    torch.manual_seed(ENC.SEED)
    pol = SwarmActorCritic(PolicyConfig.sb_train(cfg, neighbor_encoder_type="mlp")).cuda()
    env = QuadSwarmEnv(cfg)
    pcfg = PPOConfig(n_steps=8, batch_size=256, n_epochs=1)
    with pytest.raises(ValueError):
        PPOTrainer(env, pol, pcfg, update_dw="grouped")   # both updates on torch
    tr = PPOTrainer(env, pol, pcfg, seed=1, update_encoder="x3", update_tail="x3", update_dw="grouped")
    assert tr.fused_enc.runner.group is not None and tr.fused_tail.runner.group is not None and tr.collect_rollouts()
    stats = tr.train(max_updates=1)
    assert stats["n_updates"] == 1 and abs(stats["loss"]) < float("inf")
    obs, act = tr.storage.flat("obs")[:256], tr.storage.flat("actions")[:256]
    adv = torch.randn(256, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))

    def grads(fused):
        lat, tail = (tr.fused_enc.latents(obs), tr.fused_tail) if fused else (None, None)
        v, lp, _ = pol.evaluate_actions(obs, act, tail=tail, lat=lat)
        loss = -(adv * torch.exp(lp - lp.detach())).mean() + 0.5 * (v.view(-1) ** 2).mean()
        gs = torch.autograd.grad(loss, list(pol.parameters()), allow_unused=True)
        return torch.cat([(a if a is not None else torch.zeros_like(p)).flatten() for a, p in zip(gs, pol.parameters())])

    flat_f, flat_t = grads(True), grads(False)
    rel = ((flat_f - flat_t).norm() / flat_t.norm()).item()
    print(f"grouped minibatch: |g_fused - g_torch| / |g_torch| = {rel:.2e}")
    assert rel < 1e-4
    env.close()
