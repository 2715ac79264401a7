"""mha_train.attention_weight_grads -- the host step that turns the backward kernel's per-head row mixes into the four
attention weight gradients -- in fp64 on the CPU against autograd of MultiHeadAttention without its LayerNorm.  Both
sides are exact up to reassociation (bound 1e-10); a wrong transpose or head block is O(1)."""
import torch

from quadswarm_amd.mha_train import attention_weight_grads
from quadswarm_amd.ppo import MultiHeadAttention


def test_attention_weight_grads_match_autograd():
    torch.manual_seed(0)
    nh, H, B = 4, 8, 5
    m = MultiHeadAttention(nh, H, H, H).double()
    m.layer_norm = torch.nn.Identity()
    x, dy = torch.randn(B, 2, H, dtype=torch.float64), torch.randn(B, 2, H, dtype=torch.float64)
    y, s = m(x)                                                # s [B, nh, t, u]
    want = torch.autograd.grad((y * dy).sum(), [m.w_qs.weight, m.w_ks.weight, m.w_vs.weight, m.fc.weight])
    with torch.no_grad():
        X = x.reshape(2 * B, H)
        E, S = [], []
        for h in range(nh):
            blk = slice(h * H, (h + 1) * H)
            v = x @ m.w_vs.weight[blk].t()                     # [B, u, H]
            dctx = dy @ m.fc.weight[:, blk]                    # [B, t, H]
            da = dctx @ v.transpose(1, 2)                      # [B, t, u]
            ds = s[:, h] * (da - (s[:, h] * da).sum(-1, keepdim=True)) / H ** 0.5
            G = s[:, h].transpose(1, 2) @ dy                   # G[u] = sum_t s[t][u] dy_t
            R = ds @ x                                         # R[t] = sum_u ds[t][u] x_u
            E.append(G.reshape(2 * B, H).t() @ X)
            S.append(R.reshape(2 * B, H).t() @ X)
        got = attention_weight_grads(torch.stack(E), torch.stack(S), m.w_qs.weight, m.w_ks.weight, m.w_vs.weight,
                                     m.fc.weight)
    for name, g, w in zip(("w_qs", "w_ks", "w_vs", "fc"), got, want):
        assert g.shape == w.shape and (g - w).abs().max().item() <= 1e-10, name
