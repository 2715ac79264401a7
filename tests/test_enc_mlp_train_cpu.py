"""Host side of the PPO update's fused MLP-family encoders (csrc/qs_policy_enc_train.h): the new entry points' argument
checks (no device needed: they fail before any HIP call) and the packed feed_forward transposes' block order."""
import ctypes

import torch

from quadswarm_amd import _native as N
from quadswarm_amd.enc_mlp_train import FusedEncoderTrain, pack_ff_transposes
from quadswarm_amd.policy_fused import X3_SW
from quadswarm_amd.ppo import SwarmActorCritic
from test_policy_encoder_cpu import policy_config


def test_abi_argument_checks():
    L = N.lib()
    towers, trains = (N.QsEncTower * 2)(), (N.QsEncTrain * 2)()
    obs = ctypes.c_void_p(16)

    def call(bwd, stride=64, so=18, kind=N.ENC_NBR["mlp"], K=6, nd=6, od=9, B=4096, H=256, tw=towers, tr=trains, n=2, o=obs,
             grid_x=1):
        a = (o, stride, so, kind, K, nd, od, B, H, tw, tr, n)
        return L.qs_encoder_mlp_bwd_x3(*a, grid_x, None) if bwd else L.qs_encoder_mlp_train_x3(*a, None)
    for bwd in (False, True):
        for kw, msg in ((dict(o=None), b"NULL argument"), (dict(tr=None), b"NULL argument"), (dict(n=3), b"n_towers"),
                        (dict(H=64), b"hidden size"), (dict(kind=3), b"nbr_kind"), (dict(so=33), b"self features"),
                        (dict(K=11), b"1..64 wide"), (dict(kind=N.ENC_NBR["mean"], K=0), b"K >= 1"),
                        (dict(od=17), b"obstacle values"), (dict(stride=62), b"inside the obs row"),
                        (dict(B=0), b"B >= 1"), (dict(), b"NULL tower pointer")):
            assert call(bwd, **kw) == -1 and msg in L.qs_last_error(), (bwd, kw, L.qs_last_error())
    # towers complete: the train struct's pointers, then the backward's grid
    for name, _ in N.QsEncTower._fields_:
        setattr(towers[0], name, 16)
        setattr(towers[1], name, 16)
    assert call(False) == -1 and b"NULL train pointer" in L.qs_last_error()
    for name, _ in N.QsEncTrain._fields_:
        for t in trains:
            setattr(t, name, None if name == "w_fft" else 16)
    assert call(True) == -1 and b"NULL train pointer" in L.qs_last_error()   # the backward alone reads w_fft
    trains[0].w_fft = trains[1].w_fft = 16
    for g in (0, 65):   # B = 4096: 64 tiles
        assert call(True, grid_x=g) == -1 and b"grid_x" in L.qs_last_error()


def test_ff_transpose_blocks_and_param_order():
    """packed[p][ct][s][l][0][j] is f16(256 W_ff[16 s + 8 (l >> 5) + j, pH + 32 ct + (l & 31)]): part p's column block of
    the feed_forward weight, transposed to [H, 2H] (pack_mfma_weight_x3's layout of it)."""
    H = 128
    torch.manual_seed(0)
    pol = SwarmActorCritic(policy_config("mlp_obst", H))
    enc = pol.critic_encoder
    wt = pack_ff_transposes(enc)
    assert wt.shape == (3, H // 32, 2 * H // 16, 64, 2, 8) and wt.is_contiguous()
    hi = lambda x: (x.detach() * X3_SW).half()  # noqa: E731
    wff, t16 = enc.feed_forward[0].weight, wt.view(torch.float16)
    assert torch.equal(t16[2, 1, 9, 40, 0], hi(wff[16 * 9 + 8:16 * 9 + 16, 2 * H + 32 + 8]))   # the obstacle part, n = 152 ..
    assert torch.equal(t16[0, 3, 0, 5, 0, 2], hi(wff[2, 96 + 5]))                              # the self part
    ps = FusedEncoderTrain(pol).params()
    assert len(ps) == 2 * 16 and ps[16] is enc.self_encoder[0].weight and ps[31] is enc.feed_forward[0].bias
    assert ps[20] is enc.neighbor_encoder.neighbor_mlp[0].weight and ps[26] is enc.obstacle_encoder[0].weight
