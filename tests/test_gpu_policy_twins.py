"""The update's forward and the rollout's forward are the same function at the C ABI: qs_attn_embed_train_x3 /
qs_attn_pool_train_x3 (the forward with saves) and qs_attn_embed_x3 / qs_attn_pool_x3 on the same towers write
bitwise the same e2 rows, per-agent means and pooled outputs.  (The embedding is one device body; the two pooling
kernels are separate phase sequences, which nothing but this test holds to the same math -- csrc/qs_policy_x3.h,
csrc/qs_policy_train.h.)

Shapes (H, K, B): the smallest that reach every index path -- a single row; 66 rows in blocks of 60 (a block that is
not full, then 6 rows); 133 rows in blocks of 63; K = 64 (one agent per block, two blocks); both towers each."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

from quadswarm_amd import _native as NAT  # noqa: E402
from quadswarm_amd.encoder_train import _Runner, tower_params  # noqa: E402
from test_gpu_encoder_train import obs_for, random_policy  # noqa: E402

CASES = [(128, 1, 1), (256, 6, 11), (128, 7, 19), (256, 64, 2)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "H%d-K%d-B%d" % c)
def forwarded(request):
    """(runner after _Runner.forward: towers fully bound, P included; obs; the train forward's pooled outputs)"""
    H, K, B = request.param
    pol = random_policy(K, H)
    obs = obs_for(pol.cfg, B, seed=2)
    runner = _Runner(pol)
    params = [p for enc in (pol.actor_encoder, pol.critic_encoder) for p in tower_params(enc)]
    outs = runner.forward(obs, params)
    torch.cuda.synchronize()
    return runner, obs, outs


def test_rollout_embed_is_the_update_embed(forwarded):
    r, obs, _ = forwarded
    B = obs.shape[0]
    want = [(b["e2"].clone(), b["e_mean"].clone()) for b in r.buf]
    for b in r.buf:   # the rollout kernel has to write every element again
        b["e2"].fill_(float("nan"))
        b["e_mean"].fill_(float("nan"))
    NAT.check(r.L.qs_attn_embed_x3(ctypes.c_void_p(obs.data_ptr()), obs.shape[1], r.so, r.so, B, r.K, r.nd, r.H,
                                   r.towers, r.T, r.stream(obs.device)), "qs_attn_embed_x3")
    torch.cuda.synchronize()
    got = [(b["e2"].clone(), b["e_mean"].clone()) for b in r.buf]
    for b, (e2, em) in zip(r.buf, want):   # the shared forward state stays the train kernel's
        b["e2"].copy_(e2)
        b["e_mean"].copy_(em)
    for i, ((e2, em), (g2, gm)) in enumerate(zip(want, got)):
        assert torch.isfinite(e2).all() and torch.isfinite(em).all()
        assert torch.equal(g2, e2), ("e2", i, (g2 - e2).abs().max().item())
        assert torch.equal(gm, em), ("e_mean", i, (gm - em).abs().max().item())


def test_rollout_pool_is_the_update_pool(forwarded):
    r, obs, outs = forwarded
    B = obs.shape[0]
    want = [o.clone() for o in outs]
    fresh = [torch.full_like(o, float("nan")) for o in outs]
    try:
        for i in range(r.T):
            r.towers[i].out = fresh[i].data_ptr()
        NAT.check(r.L.qs_attn_pool_x3(B, r.K, r.H, r.towers, r.T, r.stream(obs.device)), "qs_attn_pool_x3")
        torch.cuda.synchronize()
    finally:
        for i in range(r.T):
            r.towers[i].out = outs[i].data_ptr()
    for i in range(r.T):
        assert torch.isfinite(want[i]).all()
        assert torch.equal(fresh[i], want[i]), ("out", i, (fresh[i] - want[i]).abs().max().item())
        assert torch.equal(outs[i], want[i])   # the train outputs were not touched
