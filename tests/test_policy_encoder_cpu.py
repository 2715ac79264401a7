"""Host side of the fused MLP-family rollout encoder (csrc/qs_policy_enc.h, qs_encoder_mlp_x3): which policies
policy_fused.encoder_supports accepts, the operand shapes pack_enc_towers hands the kernel, and the C ABI's argument checks
(no device needed: they fail before any HIP call)."""
import ctypes

import pytest
import torch

from quadswarm_amd import _native as N
from quadswarm_amd.policy_fused import X3_SW, encoder_supports, pack_enc_towers, supports
from quadswarm_amd.ppo import PolicyConfig, SwarmActorCritic

# the six configurations the kernel's branches are checked at: (neighbour encoder, so, nd, K, od)
CASES = {"none": ("no_encoder", 18, 0, 0, 0), "none_obst": ("no_encoder", 19, 6, 2, 9),      # the obstacle-offset case
         "mean": ("mean_embed", 18, 6, 6, 0), "mean_obst": ("mean_embed", 7, 3, 1, 9),
         "mlp": ("mlp", 7, 5, 7, 0), "mlp_obst": ("mlp", 19, 16, 4, 9)}                       # K nd = 35, and 64: the limit


def policy_config(case, H, **over):
    t, so, nd, K, od = CASES[case]
    kw = dict(self_obs_dim=so, neighbor_obs_dim=nd, num_use_neighbor_obs=K, obstacle_obs_dim=od, rnn_size=H,
              neighbor_hidden_size=H, obst_hidden_size=H, neighbor_encoder_type=t, act_dim=4)
    kw.update(over)
    return PolicyConfig(**kw)


REFUSED = [("mlp", dict(nonlinearity="relu")), ("mean", dict(rnn_size=64)), ("mean", dict(neighbor_hidden_size=256)),
           ("none_obst", dict(obst_hidden_size=256)), ("mlp_obst", dict(num_use_neighbor_obs=5)),   # an 80-column block
           ("mean", dict(neighbor_obs_dim=17)), ("none", dict(self_obs_dim=33)),
           ("mean", dict(neighbor_encoder_type="attention")), ("mlp_obst", dict(encoder_type="attention"))]


@pytest.mark.parametrize("case,over,ok", [(c, dict(rnn_size=H, neighbor_hidden_size=H, obst_hidden_size=H), True)
                                          for c in CASES for H in (128, 256)] + [(c, o, False) for c, o in REFUSED])
def test_encoder_supports(case, over, ok):
    pol = SwarmActorCritic(policy_config(case, 128, **over))
    assert encoder_supports(pol) == ok and not (ok and supports(pol))


def test_pack_shapes_padding_and_block_order():
    """packed[ct][s][l][0][j] is f16(256 W[32 ct + (l & 31)][16 s + 8 (l >> 5) + j]) (pack_mfma_weight_x3)."""
    H = 128
    torch.manual_seed(0)
    pol = SwarmActorCritic(policy_config("mlp_obst", H))
    w = pack_enc_towers((pol.actor_encoder, pol.critic_encoder))[1]
    ct = H // 32
    assert {k: tuple(v.shape) for k, v in w.items() if k.startswith("w_")} == {
        "w_s1p": (ct, 2, 64, 2, 8), "w_s2p": (ct, 8, 64, 2, 8), "w_n1p": (ct, 4, 64, 2, 8), "w_n2p": (ct, 8, 64, 2, 8),
        "w_n3p": (ct, 8, 64, 2, 8), "w_o1p": (ct, 1, 64, 2, 8), "w_o2p": (ct, 8, 64, 2, 8), "w_ffp": (6, ct, 8, 64, 2, 8)}
    assert all(v.is_contiguous() for v in w.values()) and w["b_ff"].shape == (2 * H,) and w["b_n3"].shape == (H,)
    enc = pol.critic_encoder
    hi = lambda x: (x.detach() * X3_SW).half()  # noqa: E731
    s1 = w["w_s1p"].view(torch.float16)
    assert torch.equal(s1[1, 1, 5, 0, :3], hi(enc.self_encoder[0].weight[37, 16:19]))   # so = 19: columns 16 .. 18
    assert not s1[1, 1, 5, :, 3:].any() and not s1[:, 1, 32:].any()                     # 19 .. 31: the padding
    o1 = w["w_o1p"].view(torch.float16)
    assert torch.equal(o1[0, 0, 35, 0, 0], hi(enc.obstacle_encoder[0].weight[3, 8])) and not o1[0, 0, 35, :, 1:].any()
    ff = w["w_ffp"].view(torch.float16)   # block (z = 1, p = 2): rows H .., the obstacle part's columns 2H ..
    assert torch.equal(ff[1 * 3 + 2, 2, 3, 40, 0], hi(enc.feed_forward[0].weight[H + 64 + 8, 2 * H + 48 + 8:2 * H + 64]))
    w = pack_enc_towers((SwarmActorCritic(policy_config("none_obst", H)).actor_encoder,))[0]   # two parts
    assert w["w_ffp"].shape[0] == 4 and "w_n1p" not in w


def test_abi_argument_checks():
    L = N.lib()
    towers = (N.QsEncTower * 2)()
    obs = ctypes.c_void_p(16)

    def call(stride=64, so=18, kind=N.ENC_NBR["mlp"], K=6, nd=6, od=9, B=4096, H=256, tw=towers, n=2, o=obs):
        return L.qs_encoder_mlp_x3(o, stride, so, kind, K, nd, od, B, H, tw, n, None)
    for kw, msg in ((dict(o=None), b"NULL argument"), (dict(tw=None), b"NULL argument"), (dict(n=3), b"n_towers"),
                    (dict(H=64), b"hidden size"), (dict(kind=3), b"nbr_kind"), (dict(so=33), b"self features"),
                    (dict(so=0), b"self features"), (dict(K=11), b"1..64 wide"),
                    (dict(kind=N.ENC_NBR["mean"], nd=17, stride=256), b"1..16 features"),
                    (dict(kind=N.ENC_NBR["mean"], K=0), b"K >= 1"), (dict(od=17), b"obstacle values"),
                    (dict(stride=62), b"inside the obs row"), (dict(kind=N.ENC_NBR["none"], stride=62), b"inside the obs row"),
                    (dict(B=0), b"B >= 1"), (dict(B=1 << 23), b"below 2^31"), (dict(), b"NULL tower pointer")):
        assert call(**kw) == -1 and msg in L.qs_last_error(), (kw, L.qs_last_error())
