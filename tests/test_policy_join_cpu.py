"""Host side of the attention families' join (csrc/qs_policy_enc.h, qs_encoder_join_x3): which policies join_supports
accepts, the C ABI's argument checks (they fail before any HIP call) and FusedRolloutPolicy's join argument."""
import ctypes

import pytest

from quadswarm_amd import _native as N
from quadswarm_amd.policy_fused import FusedRolloutPolicy, join_supports
from quadswarm_amd.ppo import PolicyConfig, SwarmActorCritic

# the three shapes the kernel is checked at: (so, nd, K, od, encoder_type)
CASES = {"attn": (18, 6, 6, 0, "mlp"), "attn_obst": (19, 6, 3, 9, "mlp"), "mha": (19, 6, 2, 9, "attention")}


def policy_config(case, H, **over):
    so, nd, K, od, et = CASES[case]
    kw = dict(self_obs_dim=so, neighbor_obs_dim=nd, num_use_neighbor_obs=K, obstacle_obs_dim=od, rnn_size=H,
              neighbor_hidden_size=H, obst_hidden_size=H, neighbor_encoder_type="attention", encoder_type=et, act_dim=4)
    kw.update(over)
    return PolicyConfig(**kw)


REFUSED = [("attn", dict(nonlinearity="relu")), ("attn", dict(rnn_size=64)), ("mha", dict(rnn_size=64)),
           ("attn", dict(neighbor_hidden_size=256)), ("attn_obst", dict(obst_hidden_size=256)), ("attn", dict(self_obs_dim=33)),
           ("attn", dict(neighbor_encoder_type="mean_embed")), ("attn_obst", dict(neighbor_encoder_type="mlp")),
           ("attn", dict(neighbor_encoder_type="no_encoder"))]


@pytest.mark.parametrize("case,over,ok", [(c, dict(rnn_size=H, neighbor_hidden_size=H, obst_hidden_size=H), True)
                                          for c in CASES for H in (128, 256)] + [(c, o, False) for c, o in REFUSED])
def test_join_supports(case, over, ok):
    assert join_supports(SwarmActorCritic(policy_config(case, 128, **over))) == ok


def test_abi_argument_checks():
    L = N.lib()
    towers = (N.QsJoinTower * 2)()
    obs = ctypes.c_void_p(16)

    def call(stride=64, so=18, oo=54, od=9, parts=1, B=4096, H=256, tw=towers, n=2, o=obs):
        return L.qs_encoder_join_x3(o, stride, so, oo, od, parts, B, H, tw, n, None)
    for kw, msg in ((dict(o=None), b"NULL argument"), (dict(tw=None), b"NULL argument"), (dict(n=3), b"n_towers"),
                    (dict(n=0), b"n_towers"), (dict(H=64), b"hidden size"), (dict(so=33), b"self features"),
                    (dict(so=0), b"self features"), (dict(od=17), b"obstacle values"), (dict(od=-1), b"obstacle values"),
                    (dict(parts=0), b"nbr_parts"), (dict(parts=3), b"nbr_parts"), (dict(oo=56), b"inside the obs row"),
                    (dict(oo=-1), b"inside the obs row"), (dict(stride=17, od=0), b"inside the obs row"),
                    (dict(B=0), b"B >= 1"), (dict(B=1 << 23), b"below 2^31"), (dict(), b"NULL tower pointer"),
                    (dict(od=0, parts=2, n=1), b"NULL tower pointer")):
        assert call(**kw) == -1 and msg in L.qs_last_error(), (kw, L.qs_last_error())


@pytest.mark.parametrize("over,precision,join", [({}, "fp32", "x3"), ({}, "x3", "bogus"), (dict(rnn_size=256), "x3", "x3")])
def test_join_argument(over, precision, join):   # (the last: a policy join_supports refuses)
    with pytest.raises(ValueError, match="join"):
        FusedRolloutPolicy(SwarmActorCritic(policy_config("attn", 128, **over)), precision, join=join)
