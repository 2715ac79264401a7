"""ppo.QuadMultiHeadAttentionEncoder (PolicyConfig.encoder_type "attention") against the reference's encoder of the
obstacle runs: tests/golden/policy_mha.{json,npz} hold the reference module's parameter names and shapes, observations
and its fp64 output with every parameter set from policy_fixture.param_value (tools/gen_golden_policy.py mha_case)."""
import json
import os

import numpy as np
import pytest
import torch

from policy_fixture import state_dict_from_names
from quadswarm_amd.ppo import PolicyConfig, QuadMultiHeadAttentionEncoder, SwarmActorCritic

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def load():
    with open(os.path.join(GOLDEN, "policy_mha.json")) as f:
        meta = json.load(f)
    data = np.load(os.path.join(GOLDEN, "policy_mha.npz"), allow_pickle=False)
    pc = PolicyConfig(self_obs_dim=meta["self_obs_dim"], neighbor_obs_dim=meta["neighbor_obs_dim"],
                      num_use_neighbor_obs=meta["num_use_neighbor_obs"], obstacle_obs_dim=meta["obstacle_obs_dim"],
                      rnn_size=meta["ref_cfg"]["rnn_size"], encoder_type="attention")
    return meta, data, pc


def test_encoder_matches_reference_fp64():
    meta, data, pc = load()
    enc = QuadMultiHeadAttentionEncoder(pc).double()
    assert list(enc.state_dict()) == meta["param_names"]
    sd = state_dict_from_names(meta["param_names"], meta["param_shapes"], torch.float32)   # fp32 values, as generated
    enc.load_state_dict({k: v.double() for k, v in sd.items()})
    with torch.no_grad():
        out = enc(torch.from_numpy(data["obs"])).numpy()
    assert out.shape == (meta["batch"], enc.out_size) and enc.out_size == 2 * pc.rnn_size
    assert np.abs(out - data["features64"]).max() < 1e-12


def test_policy_builds_the_encoder_for_both_towers_and_mlp_is_unchanged():
    _, data, pc = load()
    pol = SwarmActorCritic(pc)
    assert isinstance(pol.actor_encoder, QuadMultiHeadAttentionEncoder)
    assert isinstance(pol.critic_encoder, QuadMultiHeadAttentionEncoder)
    a, v, lp = pol(torch.from_numpy(data["obs"]).float(), deterministic=True)
    assert a.shape == (5, pc.act_dim) and v.shape == (5, 1) and bool(torch.isfinite(lp).all())
    # "mlp": the same modules in the same initialisation order as a config that never heard of the field
    kw = dict(self_obs_dim=19, neighbor_obs_dim=6, num_use_neighbor_obs=2, obstacle_obs_dim=9, rnn_size=64,
              neighbor_hidden_size=64, obst_hidden_size=64)
    torch.manual_seed(7)
    want = SwarmActorCritic(PolicyConfig(**kw)).state_dict()
    torch.manual_seed(7)
    got = SwarmActorCritic(PolicyConfig(encoder_type="mlp", **kw)).state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize("kw", [dict(obstacle_obs_dim=0), dict(obstacle_obs_dim=9, num_use_neighbor_obs=0)])
def test_attention_encoder_needs_obstacles_and_neighbours(kw):
    with pytest.raises(ValueError):
        SwarmActorCritic(PolicyConfig(encoder_type="attention", **kw))
