"""Fused rollout forward of the attention policy: the no-grad evaluation that SB3's
collect_rollouts makes of ActorCriticPolicyCustomSeparateWeights (swarm_rl/models/ActorCriticPolicyCustom.py:
515-536) once per step, with both towers' attention neighbour encoders (QuadNeighborhoodEncoderAttention,
swarm_rl/models/quad_multi_model.py:44-101) run by the HIP kernels of csrc/qs_policy.h through the C ABI
(qs_attn_embed / qs_attn_pool) instead of ~20 torch GEMM + tanh launches per tower.

Per step, for the actor and the critic tower at once (one launch per stage):
  HIP     e1 (self and neighbour halves of layer 0), e2 rows, mean_K(e2)   (qs_attn_embed)
  HIP     P = mean_K(e2) W_a1[:, H:]^T + b_a1 (x3, H 256; else torch)   [B, H]
  HIP     value path, attention path, softmax over K, pooled out    (qs_attn_pool)
  torch   self encoder, feed_forward, core, decoder, heads          (small per-agent GEMMs; tail="x3": below)
The result is the same function as the torch module (fp32 throughout; only the summation order of the
GEMMs differs: tests/test_gpu_policy_fused.py bounds it).  Training (the PPO update with autograd) keeps
the torch module.

A policy built with encoder_type "attention" (the obstacle runs' QuadMultiHeadAttentionEncoder, quad_multi_model.py:
125-200) is the second family: with precision "x3" one launch of qs_mha_encoder_x3 (csrc/qs_policy_mha.h) takes both
towers from the observations to the two normalised attention tokens per agent; the self encoder and feed_forward
stay in torch (the self encoder's second layer on qs_linear_tanh_x3 where it fits).  tests/test_gpu_policy_mha.py.

A QuadMultiEncoder whose neighbour encoder is a plain MLP (mean_embed, mlp, or none) is the third family
(encoder_supports): with precision "x3" one launch of qs_encoder_mlp_x3 (csrc/qs_policy_enc.h) takes both towers from
the observations to the feed_forward output, so with tail "x3" a rollout step is two launches.
tests/test_gpu_policy_encoder.py.

tail="x3" (any family): everything after the feed_forward -- core, decoder, action_net / value_net, the squashed
Gaussian's sampling and log-prob -- is one launch of qs_policy_tail_x3 (csrc/qs_policy_tail.h) for both towers in place
of the torch row above.  tests/test_gpu_policy_tail.py.

join="x3" (the two attention families, join_supports): the self encoder, the obstacle encoder and the feed_forward --
what lies between the neighbour kernels and the tail -- are one launch of qs_encoder_join_x3 (csrc/qs_policy_enc.h
enc_join_x3_kernel) for both towers, reading the neighbour kernels' rows in place; with tail "x3" a step of either
family then issues no torch GEMM.  tests/test_gpu_policy_join.py.
"""
import ctypes

import torch

from . import _native as NAT


def pack_mfma_weight(w):
    """[N, Kd] fp32 weight -> the matrix-core operand layout of qs_attn_tower (quadswarm.h):
    packed[ct][g][l][u] = W[32 ct + (l & 31)][(l >> 5) Kd/2 + 4 g + u]."""
    n, kd = w.shape
    assert n % 32 == 0 and kd % 8 == 0, (n, kd)
    return w.detach().float().contiguous().view(n // 32, 32, 2, kd // 8, 4).permute(0, 3, 2, 1, 4).contiguous()


X3_SW = 256.0   # weight scale of the split-f16 packing (csrc/qs_policy_x3.h X3_SW)
X3_SX = 256.0   # activation scale of the x3 tiles (csrc/qs_policy_x3.h X3_SX)
X3_SIN = 16.0   # raw-observation scale of the x3 layer-0 inputs (csrc/qs_policy_x3.h X3_SIN)
F16_MAX = 65504.0
X3_SC = 16.0    # context scale of the multi-head attention encoder (csrc/qs_policy_mha.h X3_SC)
MHA_NBW, MHA_OBW = 64, 16   # its layer-0 columns: the neighbour block, the obstacle values (csrc/qs_policy_mha.h)


def pack_mfma_weight_x3(w):
    """[N, Kd] fp32 weight -> the split-f16 operand layout of qs_attn_embed_x3 / qs_attn_pool_x3 (quadswarm.h):
    packed[ct][s][l] = 8 halves of hi(256 W[32 ct + (l & 31)][16 s + 8 (l >> 5) + j]), then the 8 lo halves,
    hi = f16(256 w), lo = f16(256 w - hi).  Returned as an int16 tensor [N/32, Kd/16, 64, 2, 8].
    Raises ValueError for a weight with |256 w| beyond the f16 range (it would pack as +-inf)."""
    n, kd = w.shape
    assert n % 32 == 0 and kd % 16 == 0, (n, kd)
    ws = w.detach().float() * X3_SW
    if not bool(ws.abs().amax() < F16_MAX):   # NaN fails too
        raise ValueError(f"x3 packing: max |w| = {float(w.detach().abs().amax()):.4g} is outside the split-f16 range "
                         f"(< {F16_MAX / X3_SW:.4g})")
    hi = ws.half()
    lo = (ws - hi.float()).half()

    def lay(x):   # [n, kd] -> [ct, s, h, r, j] -> [ct, s, l = 32 h + r, j]
        return x.contiguous().view(n // 32, 32, kd // 16, 2, 8).permute(0, 2, 3, 1, 4).reshape(n // 32, kd // 16, 64, 8)
    return torch.stack((lay(hi), lay(lo)), dim=3).contiguous().view(torch.int16)


def pack_mfma_weights_x3(ws):
    """pack_mfma_weight_x3 of several weights at once: those of one shape packed as one batch, the range of all of
    them checked with one host read (the update packs 22 matrices per minibatch).  Same layout, same ValueError."""
    groups = {}
    for i, w in enumerate(ws):
        groups.setdefault(tuple(w.shape), []).append(i)
    out = [None] * len(ws)
    scaled = {}
    peak = []
    for shape, idx in groups.items():
        n, kd = shape
        assert n % 32 == 0 and kd % 16 == 0, shape
        x = torch.stack([ws[i].detach().float() for i in idx]) * X3_SW
        scaled[shape] = x
        peak.append(x.abs().amax())
    if not bool(torch.stack(peak).amax() < F16_MAX):   # NaN fails too
        m = max(float(w.detach().abs().amax()) for w in ws)
        raise ValueError(f"x3 packing: max |w| = {m:.4g} is outside the split-f16 range (< {F16_MAX / X3_SW:.4g})")
    for shape, idx in groups.items():
        n, kd = shape
        x = scaled[shape]
        hi = x.half()
        lo = (x - hi.float()).half()
        g = len(idx)

        def lay(t):   # [g, n, kd] -> [g, ct, s, h, r, j] -> [g, ct, s, l = 32 h + r, j]
            return t.view(g, n // 32, 32, kd // 16, 2, 8).permute(0, 1, 3, 4, 2, 5).reshape(g, n // 32, kd // 16, 64, 8)
        packed = torch.stack((lay(hi), lay(lo)), dim=4).contiguous().view(torch.int16)
        for j, i in enumerate(idx):
            out[i] = packed[j]
    return out


def pack_linear_x3(w):
    """[N, K] fp32 weight (N a multiple of 256, K 256 or 512) -> the operand of qs_linear_tanh_x3: the packs of its
    256 x 256 blocks W[256 z .., 256 p ..] in (z, p) order, one contiguous int16 tensor.  ValueError out of range."""
    n, k = w.shape
    assert n % 256 == 0 and k in (256, 512), (n, k)
    blocks = [w[256 * z:256 * (z + 1), 256 * p:256 * (p + 1)] for z in range(n // 256) for p in range(k // 256)]
    return torch.stack(pack_mfma_weights_x3(blocks)).contiguous()


def ff_supported(lin):
    """Can qs_linear_tanh_x3 evaluate this feed_forward Linear?"""
    return lin.in_features in (256, 512) and lin.out_features % 256 == 0 and 256 <= lin.out_features <= 1024


def self_l2_supported(se):
    """The self encoder's second Linear + Tanh (Sequential(Linear, Tanh, Linear, Tanh), tanh inputs) on
    qs_linear_tanh_x3?"""
    return (len(se) == 4 and isinstance(se[1], torch.nn.Tanh) and isinstance(se[3], torch.nn.Tanh)
            and isinstance(se[2], torch.nn.Linear) and ff_supported(se[2]))


def linear_tanh_x3(x, packed, bias, out=None):
    """tanh(x W^T + b) for x [M, K] (|x| <= 1: tanh outputs) on the split-f16 matrix cores (qs_linear_tanh_x3)."""
    M, K = x.shape
    N = bias.shape[0]
    y = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=x.device)
    st = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    assert x.is_contiguous() and packed.is_contiguous() and bias.is_contiguous() and y.is_contiguous()
    NAT.check(NAT.lib().qs_linear_tanh_x3(ctypes.c_void_p(x.data_ptr()), M, K, ctypes.c_void_p(packed.data_ptr()),
                                          packed.numel() * packed.element_size(), ctypes.c_void_p(bias.data_ptr()),
                                          ctypes.c_void_p(y.data_ptr()), N, st),
              "qs_linear_tanh_x3")
    return y


def linear_tanh_cat_x3(x0, x1, packed, bias, out=None):
    """tanh([x0 | x1] W^T + b) for x0, x1 [M, 256] (|x| <= 1) without forming the concatenation (qs_linear_tanh_cat_x3);
    packed = pack_linear_x3(W) for W [N, 512]."""
    M = x0.shape[0]
    N = bias.shape[0]
    assert x0.shape == (M, 256) and x1.shape == (M, 256)
    y = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=x0.device)
    assert x0.is_contiguous() and x1.is_contiguous() and packed.is_contiguous() and bias.is_contiguous() and y.is_contiguous()
    st = ctypes.c_void_p(torch.cuda.current_stream(x0.device).cuda_stream)
    NAT.check(NAT.lib().qs_linear_tanh_cat_x3(ctypes.c_void_p(x0.data_ptr()), ctypes.c_void_p(x1.data_ptr()), M,
                                              ctypes.c_void_p(packed.data_ptr()), packed.numel() * packed.element_size(),
                                              ctypes.c_void_p(bias.data_ptr()), ctypes.c_void_p(y.data_ptr()), N, st),
              "qs_linear_tanh_cat_x3")
    return y


def cat_free(parts):
    """Two contiguous [M, 256] parts: qs_linear_tanh_cat_x3 reads them in place of their concatenation."""
    return (len(parts) == 2 and all(p.dim() == 2 and p.shape[1] == 256 and p.is_contiguous() for p in parts)
            and parts[0].shape[0] == parts[1].shape[0])


def linear_bias_x3(x, packed, bias, out=None):
    """x W^T + b for x [M, K] (|x| <= 1) on the split-f16 matrix cores (qs_linear_bias_x3: qs_linear_tanh_x3 without
    the tanh); the attention score layer's mean half P = e_mean A_m^T + b_a1."""
    M, K = x.shape
    N = bias.shape[0]
    y = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=x.device)
    assert x.is_contiguous() and packed.is_contiguous() and bias.is_contiguous() and y.is_contiguous()
    st = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    NAT.check(NAT.lib().qs_linear_bias_x3(ctypes.c_void_p(x.data_ptr()), M, K, ctypes.c_void_p(packed.data_ptr()),
                                          packed.numel() * packed.element_size(), ctypes.c_void_p(bias.data_ptr()),
                                          ctypes.c_void_p(y.data_ptr()), N, st),
              "qs_linear_bias_x3")
    return y


def linear_rows_x3(x, row_scale, packed, n_out, out=None):
    """x W^T for rows x [M, K] of any magnitude (their power-of-two scales row_scale [M]: _pow2_scales of the row
    maxima) on the split-f16 matrix cores (qs_linear_rows_x3); packed = pack_linear_x3(W) for W [n_out, K]."""
    M, K = x.shape
    y = out if out is not None else torch.empty(M, n_out, dtype=torch.float32, device=x.device)
    assert x.is_contiguous() and row_scale.is_contiguous() and packed.is_contiguous() and y.is_contiguous()
    st = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    NAT.check(NAT.lib().qs_linear_rows_x3(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(row_scale.data_ptr()), M, K,
                                          ctypes.c_void_p(packed.data_ptr()), packed.numel() * packed.element_size(),
                                          ctypes.c_void_p(y.data_ptr()), n_out, st),
              "qs_linear_rows_x3")
    return y


def supports(policy):
    """Can the fused kernels evaluate this policy's encoders?"""
    c = policy.cfg
    if c.encoder_type == "attention":   # QuadMultiHeadAttentionEncoder on qs_mha_encoder_x3 (csrc/qs_policy_mha.h)
        return (c.nonlinearity == "tanh" and c.rnn_size in (128, 256) and
                1 <= c.neighbor_obs_dim * c.num_use_neighbor_obs <= MHA_NBW and 1 <= c.obstacle_obs_dim <= MHA_OBW)
    return (c.neighbor_encoder_type == "attention" and c.num_use_neighbor_obs >= 1 and
            c.neighbor_hidden_size in (128, 256) and 1 <= c.neighbor_obs_dim <= 16 and
            c.num_use_neighbor_obs <= 64 and c.self_obs_dim + c.neighbor_obs_dim <= 32 and c.nonlinearity == "tanh")


ENC_SW, ENC_NBW, ENC_NDW, ENC_OBW = 32, 64, 16, 16   # layer-0 contraction widths of qs_encoder_mlp_x3 (csrc/qs_policy_enc.h)


def enc_nbr_kind(cfg):
    """The neighbour branch qs_encoder_mlp_x3 evaluates for an encoder_type "mlp" policy: "none", "mean", "mlp", or
    None for a neighbour encoder it does not have (attention)."""
    if cfg.num_use_neighbor_obs == 0 or cfg.neighbor_encoder_type == "no_encoder":
        return "none"
    return {"mean_embed": "mean", "mlp": "mlp"}.get(cfg.neighbor_encoder_type)


def encoder_supports(policy):
    """Can qs_encoder_mlp_x3 (csrc/qs_policy_enc.h) evaluate this policy's encoders, observations to feed_forward
    output?  QuadMultiEncoder with the mean_embed, mlp or no neighbour encoder; tanh; every branch rnn_size (128 or 256)
    wide; self <= 32, the mlp block <= 64, one mean_embed neighbour <= 16 and the obstacle values <= 16 columns."""
    c = policy.cfg
    kind = enc_nbr_kind(c) if c.encoder_type == "mlp" else None
    if kind is None or c.nonlinearity != "tanh" or c.rnn_size not in (128, 256):
        return False
    if kind != "none" and c.neighbor_hidden_size != c.rnn_size:
        return False
    if c.obstacle_obs_dim and c.obst_hidden_size != c.rnn_size:
        return False
    if kind == "mlp" and not 1 <= c.neighbor_obs_dim * c.num_use_neighbor_obs <= ENC_NBW:
        return False
    if kind == "mean" and not 1 <= c.neighbor_obs_dim <= ENC_NDW:
        return False
    return 1 <= c.self_obs_dim <= ENC_SW and 0 <= c.obstacle_obs_dim <= ENC_OBW


def enc_tower_mats(enc):
    """One QuadMultiEncoder tower's matrices as qs_enc_tower takes them, before packing: {name: [N, Kd] fp32}, each
    branch's layer 0 zero-padded to its contraction width, and "w_ffp" the list of the feed_forward's H x H blocks
    W[zH:(z+1)H, pH:(p+1)H] in (z, p) order."""
    c, H = enc.cfg, enc.cfg.rnn_size

    def pad(w, width):
        out = torch.zeros(H, width, dtype=torch.float32, device=w.device)
        out[:, :w.shape[1]] = w.detach()
        return out
    se = enc.self_encoder
    m = dict(w_s1p=pad(se[0].weight, ENC_SW), w_s2p=se[2].weight)
    kind = enc_nbr_kind(c)
    if kind == "mlp":
        nm = enc.neighbor_encoder.neighbor_mlp
        m.update(w_n1p=pad(nm[0].weight, ENC_NBW), w_n2p=nm[2].weight, w_n3p=nm[4].weight)
    elif kind == "mean":
        em = enc.neighbor_encoder.embedding_mlp
        m.update(w_n1p=pad(em[0].weight, ENC_NDW), w_n2p=em[2].weight)
    if enc.obstacle_encoder is not None:
        oe = enc.obstacle_encoder
        m.update(w_o1p=pad(oe[0].weight, ENC_OBW), w_o2p=oe[2].weight)
    wff = enc.feed_forward[0].weight
    assert wff.shape[0] == 2 * H and wff.shape[1] % H == 0
    m["w_ffp"] = [wff[z * H:(z + 1) * H, p * H:(p + 1) * H] for z in range(2) for p in range(wff.shape[1] // H)]
    return m


def enc_tower_biases(enc):
    c = enc.cfg
    se = enc.self_encoder
    b = dict(b_s1=se[0].bias, b_s2=se[2].bias, b_ff=enc.feed_forward[0].bias)
    kind = enc_nbr_kind(c)
    if kind == "mlp":
        nm = enc.neighbor_encoder.neighbor_mlp
        b.update(b_n1=nm[0].bias, b_n2=nm[2].bias, b_n3=nm[4].bias)
    elif kind == "mean":
        em = enc.neighbor_encoder.embedding_mlp
        b.update(b_n1=em[0].bias, b_n2=em[2].bias)
    if enc.obstacle_encoder is not None:
        b.update(b_o1=enc.obstacle_encoder[0].bias, b_o2=enc.obstacle_encoder[2].bias)
    return {k: v.detach().contiguous() for k, v in b.items()}


def pack_enc_towers(encs, tower_mats=enc_tower_mats, tower_biases=enc_tower_biases):
    """Every tower's qs_enc_tower operands: the matrices of enc_tower_mats packed in one pack_mfma_weights_x3 batch (the
    feed_forward's blocks stacked, contiguous) plus the bias vectors.  ValueError for a weight out of the f16 range.
    (tower_mats / tower_biases: the join's, pack_join_towers.)"""
    mats = [tower_mats(enc) for enc in encs]
    flat, where = [], []
    for i, m in enumerate(mats):
        for name, w in m.items():
            for w1 in (w if name == "w_ffp" else [w]):
                flat.append(w1)
                where.append((i, name))
    pk = pack_mfma_weights_x3(flat)
    out = [tower_biases(enc) for enc in encs]
    for (i, name), t in zip(where, pk):
        if name == "w_ffp":
            out[i].setdefault(name, []).append(t)
        else:
            out[i][name] = t.contiguous()
    for w in out:
        w["w_ffp"] = torch.stack(w["w_ffp"]).contiguous()
    return out


def _join_self(enc):
    """The self branch of an attention-family encoder: QuadMultiEncoder's self_encoder, the multi-head family's
    self_embed_layer."""
    return enc.self_embed_layer if enc.cfg.encoder_type == "attention" else enc.self_encoder


def join_supports(policy):
    """Can qs_encoder_join_x3 (csrc/qs_policy_enc.h enc_join_x3_kernel) evaluate what follows this policy's neighbour
    kernels -- self encoder, obstacle encoder, feed_forward -- in one launch?  A policy supports() accepts; tanh; rnn_size
    128 or 256; the self encoder two Linear + Tanh of that width; the pooled neighbour row and the obstacle branch of that
    width too (QuadMultiEncoder); self <= 32 and obstacle <= 16 columns."""
    c = policy.cfg
    if not supports(policy) or c.nonlinearity != "tanh" or c.rnn_size not in (128, 256):
        return False
    if not (1 <= c.self_obs_dim <= ENC_SW and 0 <= c.obstacle_obs_dim <= ENC_OBW):
        return False
    se = _join_self(policy.actor_encoder)
    if not (len(se) == 4 and all(isinstance(se[i], torch.nn.Linear) and isinstance(se[i + 1], torch.nn.Tanh) and
                                 se[i].out_features == c.rnn_size for i in (0, 2))):
        return False
    if c.encoder_type == "attention":   # [self | token 0 | token 1], the obstacle values inside the tokens
        return True
    return c.neighbor_hidden_size == c.rnn_size and (not c.obstacle_obs_dim or c.obst_hidden_size == c.rnn_size)


def join_tower_mats(enc):
    """enc_tower_mats for qs_join_tower: the self branch, the obstacle branch (QuadMultiEncoder with obstacles) and the
    feed_forward's H x H blocks in (z, p) order over the parts [self | pooled | obstacle] or [self | token 0 | token 1]."""
    if enc.cfg.encoder_type != "attention":
        return enc_tower_mats(enc)   # (its neighbour kinds do not include attention: self, obstacle and blocks only)
    H, se = enc.cfg.rnn_size, enc.self_embed_layer
    w_s1 = torch.zeros(H, ENC_SW, dtype=torch.float32, device=se[0].weight.device)
    w_s1[:, :se[0].in_features] = se[0].weight.detach()
    wff = enc.feed_forward[0].weight
    assert wff.shape == (2 * H, 3 * H)
    return dict(w_s1p=w_s1, w_s2p=se[2].weight,
                w_ffp=[wff[z * H:(z + 1) * H, p * H:(p + 1) * H] for z in range(2) for p in range(3)])


def join_tower_biases(enc):
    if enc.cfg.encoder_type != "attention":
        return enc_tower_biases(enc)
    se = enc.self_embed_layer
    return {k: v.detach().contiguous() for k, v in dict(b_s1=se[0].bias, b_s2=se[2].bias, b_ff=enc.feed_forward[0].bias).items()}


def pack_join_towers(encs):
    """Every tower's qs_join_tower weights and biases: one pack_mfma_weights_x3 batch, one host read.  ValueError for a
    weight out of the f16 range."""
    return pack_enc_towers(encs, join_tower_mats, join_tower_biases)


def join_token_bound(encs):
    """max |token element| of the multi-head family: a LayerNorm output is at most sqrt(H) |ln_g| + |ln_b| (|x_hat| <
    sqrt(H)).  One host read."""
    lns = [enc.attention_layer.layer_norm for enc in encs]
    g = torch.stack([ln.weight.detach().abs().amax() for ln in lns]).amax()
    b = torch.stack([ln.bias.detach().abs().amax() for ln in lns]).amax()
    return float(g * lns[0].normalized_shape[0] ** 0.5 + b)


def tail_chain(core, decoder):
    """The Linear layers of a tower's core followed by its decoder's: the chain qs_policy_tail_x3 evaluates."""
    return [m for m in list(core) + list(decoder) if isinstance(m, torch.nn.Linear)]


def tail_supports(policy):
    """Can qs_policy_tail_x3 evaluate this policy's core, decoder, heads and action distribution?  tanh layers, all
    of width rnn_size (128 or 256) after the 2 rnn_size wide feed_forward, at most 8 of them, act_dim <= 8."""
    c = policy.cfg
    full = c.rnn_type == "full" and c.rnn_num_layers > 0
    n = (c.rnn_num_layers if full else 0) + len(c.decoder_mlp_layers)
    return (c.nonlinearity == "tanh" and c.rnn_size in (128, 256) and n <= NAT.TAIL_MAX_LAYERS and
            all(d == c.rnn_size for d in c.decoder_mlp_layers) and 1 <= c.act_dim <= NAT.TAIL_MAX_OUT and
            policy.actor_encoder.out_size == 2 * c.rnn_size)


def mha_weight_range(encs):
    """(max |w| over the multi-head attention encoders' matrices the kernels pack, max_row |w_vs|_1): the two numbers the
    split-f16 range rules bound (|w| < 255.9; |ctx| <= max_row |w_vs|_1 < 65504 / X3_SC).  One host read."""
    stats = []
    for enc in encs:
        at = enc.attention_layer
        ms = (enc.neighbor_embed_layer[0], enc.neighbor_embed_layer[2], enc.obstacle_embed_layer[0],
              enc.obstacle_embed_layer[2], at.w_qs, at.w_ks, at.w_vs, at.fc)
        stats.append(torch.stack((torch.stack([m.weight.detach().abs().amax() for m in ms]).amax(),
                                  at.w_vs.weight.detach().abs().sum(dim=1).amax())))
    return torch.stack(stats).amax(dim=0).tolist()


def mha_range_ok(big, vnorm):
    return big < F16_MAX / X3_SW and vnorm < F16_MAX / X3_SC   # NaN fails too


def pack_mha_tower(enc, H, nbw, od, transposes=False):
    """One tower's qs_mha_tower operands (quadswarm.h): the packed weights and the bias / LayerNorm vectors.
    transposes: also the backward's W^T operands (qs_mha_train w_*tp), packed in the same batch."""
    ne, oe, at = enc.neighbor_embed_layer, enc.obstacle_embed_layer, enc.attention_layer
    w_e1 = torch.zeros(H, MHA_NBW + MHA_OBW, dtype=torch.float32, device=ne[0].weight.device)
    w_e1[:, :nbw] = ne[0].weight.detach()                       # [neighbour block | 0 | obstacle values | 0]
    w_e1[:, MHA_NBW:MHA_NBW + od] = oe[0].weight.detach()
    rows = lambda lin: [lin.weight[h * H:(h + 1) * H] for h in range(4)]  # noqa: E731  head h's projection
    fcs = [at.fc.weight[:, h * H:(h + 1) * H] for h in range(4)]
    mats = [w_e1, ne[2].weight, oe[2].weight] + rows(at.w_qs) + rows(at.w_ks) + rows(at.w_vs) + fcs   # 18 [H, H]: one batch
    if transposes:
        mats += [m.t() for m in mats[1:]]
    pk = pack_mfma_weights_x3(mats)
    w = dict(w_e1p=pk[0], w_n2p=pk[1], w_o2p=pk[2], w_qp=torch.stack(pk[3:7]), w_kp=torch.stack(pk[7:11]),
             w_vp=torch.stack(pk[11:15]), w_fcp=torch.stack(pk[15:19]),
             b_n1=ne[0].bias.detach(), b_o1=oe[0].bias.detach(), b_n2=ne[2].bias.detach(),
             b_o2=oe[2].bias.detach(), ln_g=at.layer_norm.weight.detach(), ln_b=at.layer_norm.bias.detach())
    if transposes:
        w.update(w_n2tp=pk[19], w_o2tp=pk[20], w_qtp=torch.stack(pk[21:25]), w_ktp=torch.stack(pk[25:29]),
                 w_vtp=torch.stack(pk[29:33]), w_fctp=torch.stack(pk[33:37]))
    return w


MHA_TOWER_FIELDS = ("w_e1p", "b_n1", "b_o1", "w_n2p", "w_o2p", "b_n2", "b_o2", "w_qp", "w_kp", "w_vp", "w_fcp", "ln_g", "ln_b")


class FusedRolloutPolicy:
    """forward(obs) / predict_values(obs) of a SwarmActorCritic with the fused neighbour encoders.
    refresh() re-packs the weights: call it whenever the policy's parameters changed (PPOTrainer does,
    once per rollout)."""

    PRECISIONS = ("fp32", "x3")
    TAILS = ("torch", "x3")

    JOINS = ("torch", "x3")

    def __init__(self, policy, precision="fp32", tail="torch", join="torch"):
        """precision "fp32": fp32 operands on the fp32 matrix cores (v_mfma_f32_32x32x2f32); "x3": every fp32 product
        as three f16 products (hi/lo split, fp32 accumulation, ~7e-7 relative per product) on the f16 matrix cores
        (csrc/qs_policy_x3.h), 5.3x the contraction rate.
        tail "torch": core, decoder, heads and the action distribution as torch launches; "x3": as one launch of
        qs_policy_tail_x3 (csrc/qs_policy_tail.h; the chain's products split like precision "x3", the heads fp32).
        join (the attention families, precision "x3"): what lies between the neighbour kernels and the tail -- self
        encoder, obstacle encoder, feed_forward -- "torch": as torch and single-layer launches; "x3": as one launch of
        qs_encoder_join_x3 (csrc/qs_policy_enc.h) that reads the neighbour kernels' rows in place."""
        if precision not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {self.PRECISIONS}")
        if tail not in self.TAILS:
            raise ValueError(f"tail must be one of {self.TAILS}")
        if join not in self.JOINS:
            raise ValueError(f"join must be one of {self.JOINS}")
        if join == "x3" and not (precision == "x3" and join_supports(policy)):
            raise ValueError("fused rollout join: needs precision 'x3' and a policy join_supports accepts (an attention "
                             "family with tanh branches of width rnn_size 128 or 256)")
        self.join_mode = join
        self.packed_join = None        # what refresh() packed for the x3 join; None: the torch join evaluates
        self.join_towers = (NAT.QsJoinTower * NAT.ATTN_MAX_TOWERS)()
        self.join_out = None
        if tail == "x3" and not tail_supports(policy):
            raise ValueError("fused rollout tail: needs tanh core / decoder layers of width rnn_size (128 or 256), at "
                             "most 8 of them, and act_dim <= 8")
        self.tail_mode = tail
        self.packed_tail = None        # what refresh() packed for the x3 tail; None: the torch tail evaluates
        self.tail_towers = (NAT.QsTailTower * NAT.ATTN_MAX_TOWERS)()
        self.precision = precision
        self.packed_precision = None   # what refresh() packed: precision, or fp32 when x3 weights are out of range
        self._obs_absmax = None        # running max |obs| the x3 layer 0 has seen since the last check_inputs()
        # the MLP family (QuadMultiEncoder with the mean_embed, mlp or no neighbour encoder, csrc/qs_policy_enc.h): x3 only
        self.enc = not supports(policy) and encoder_supports(policy)
        if not supports(policy) and not self.enc:
            raise ValueError("fused rollout forward: needs the tanh attention encoder with hidden size 128 or 256")
        self.policy = policy
        self.cfg = policy.cfg
        # the multi-head attention encoder family (encoder_type "attention", csrc/qs_policy_mha.h): x3 only
        self.mha = self.cfg.encoder_type == "attention"
        self.H = self.cfg.rnn_size if self.mha or self.enc else self.cfg.neighbor_hidden_size
        self.K = self.cfg.num_use_neighbor_obs
        self.nd = self.cfg.neighbor_obs_dim
        self.so = self.cfg.self_obs_dim
        self.encs = (policy.actor_encoder, policy.critic_encoder)
        self.L = NAT.lib()
        self.B = None
        self.packed = None
        tower = NAT.QsEncTower if self.enc else NAT.QsMhaTower if self.mha else NAT.QsAttnTower
        self.towers = (tower * NAT.ATTN_MAX_TOWERS)()

    # ---- weights / buffers ----
    def refresh(self):
        """Re-pack the weights.  x3: a weight outside the split-f16 range (|w| >= 255.9) would become +-inf; the
        towers are then packed (and evaluated) in fp32 until a later refresh finds every weight in range again."""
        if self.tail_mode == "x3":
            self._refresh_tail()
        if self.join_mode == "x3":
            self._refresh_join()
        if self.mha:
            return self._refresh_mha()
        if self.enc:
            return self._refresh_enc()
        prec = self.precision
        if prec == "x3":
            lim = F16_MAX / X3_SW
            big = max(float(m.weight.detach().abs().amax()) for enc in self.encs
                      for m in (enc.neighbor_encoder.embedding_mlp[0], enc.neighbor_encoder.embedding_mlp[2],
                                enc.neighbor_encoder.neighbor_value_mlp[0], enc.neighbor_encoder.neighbor_value_mlp[2],
                                enc.neighbor_encoder.attention_mlp[0], enc.neighbor_encoder.attention_mlp[2]))
            if not big < lim:
                import warnings
                warnings.warn(f"x3 rollout encoders: max |w| = {big:.4g} >= {lim:.4g} (f16 range); packing fp32")
                prec = "fp32"
        self.packed_precision = prec
        self._pack(prec)

    def check_inputs(self):
        """x3 only: raise if an observation given to the encoders since the last call was beyond the split-f16 range
        of layer 0 (|obs| >= 4094 packs as +-inf), i.e. the outputs of those calls are not the fp32 function.
        Non-finite observations are left to the env's non-finite guard.  One host sync (PPOTrainer: per rollout)."""
        m, self._obs_absmax = self._obs_absmax, None
        if m is None:
            return
        v = float(m)
        if v == v and v != float("inf") and v * X3_SIN >= F16_MAX:
            raise ValueError(f"x3 rollout encoders: an observation reached |obs| = {v:.4g} >= {F16_MAX / X3_SIN:.4g}, "
                             "beyond the split-f16 range of layer 0; use rollout_precision='fp32'")

    def _pack(self, prec):
        H, so = self.H, self.so
        pack = pack_mfma_weight_x3 if prec == "x3" else pack_mfma_weight
        packed = []
        for enc in self.encs:
            ne = enc.neighbor_encoder
            emb, val, att = ne.embedding_mlp, ne.neighbor_value_mlp, ne.attention_mlp
            w0 = emb[0].weight.detach()
            w_e1 = torch.zeros(H, 32, dtype=torch.float32, device=w0.device)   # [neighbour | self | 0]
            w_e1[:, :self.nd] = w0[:, so:]
            w_e1[:, self.nd:self.nd + so] = w0[:, :so]
            packed.append(dict(
                w_e1p=pack(w_e1), b_e1=emb[0].bias.detach(),
                w_e2p=pack(emb[2].weight), b_e2=emb[2].bias.detach(),
                w_v1p=pack(val[0].weight), b_v1=val[0].bias.detach(),
                w_v2p=pack(val[2].weight), b_v2=val[2].bias.detach(),
                w_a1ep=pack(att[0].weight[:, :H]), w_a1m=att[0].weight[:, H:].detach().contiguous(),
                b_a1=att[0].bias.detach().contiguous(),
                w_a2p=pack(att[2].weight), b_a2=att[2].bias.detach(),
                w_a3=att[4].weight.detach().reshape(-1).contiguous(), b_a3=float(att[4].bias.detach().item())))
            if prec == "x3" and H == 256:   # P = e_mean A_m^T + b_a1 on qs_linear_bias_x3 (|e_mean| <= 1)
                packed[-1].update(w_a1mp=pack_linear_x3(att[0].weight[:, H:].detach()))
            if self.packed_join is not None:   # the join kernel evaluates these layers: nothing to pack for the torch join
                continue
            ff = enc.feed_forward[0]
            if prec == "x3" and ff_supported(ff) and float(ff.weight.detach().abs().amax()) < F16_MAX / X3_SW:
                packed[-1].update(w_ffp=pack_linear_x3(ff.weight.detach()), b_ff=ff.bias.detach().contiguous())
            se = enc.self_encoder
            if (prec == "x3" and self_l2_supported(se)
                    and float(se[2].weight.detach().abs().amax()) < F16_MAX / X3_SW):
                packed[-1].update(w_s2p=pack_linear_x3(se[2].weight.detach()), b_s2=se[2].bias.detach().contiguous())
        self.packed = packed
        self._bind()

    def _alloc(self, B, dev):
        H, K, T = self.H, self.K, len(self.encs)
        z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        self.B = B
        self.P = z(T, B, H)
        self.e2, self.e_mean, self.out = z(T, B * K, H), z(T, B, H), z(T, B, H)
        self._bind()

    def _bind(self):
        if self.packed is None or self.B is None:
            return
        p = lambda t: t.data_ptr()  # noqa: E731
        for i, w in enumerate(self.packed):
            t = self.towers[i]
            t.w_e1p, t.b_e1 = p(w["w_e1p"]), p(w["b_e1"])
            t.w_e2p, t.b_e2 = p(w["w_e2p"]), p(w["b_e2"])
            t.e2, t.e_mean, t.P = p(self.e2[i]), p(self.e_mean[i]), p(self.P[i])
            t.w_v1p, t.b_v1, t.w_v2p, t.b_v2 = p(w["w_v1p"]), p(w["b_v1"]), p(w["w_v2p"]), p(w["b_v2"])
            t.w_a1ep, t.w_a2p, t.b_a2, t.w_a3 = p(w["w_a1ep"]), p(w["w_a2p"]), p(w["b_a2"]), p(w["w_a3"])
            t.b_a3, t.out = w["b_a3"], p(self.out[i])

    # ---- the multi-head attention encoder family ----
    def _refresh_mha(self):
        """precision "fp32": the torch module evaluates this family (it has no fp32-MFMA kernels).  "x3": the kernel,
        unless a weight is outside the split-f16 range (|w| >= 255.9) or the context bound max_row |w_vs|_1 (|ctx| <=
        it, since the tokens are tanh outputs) reaches 65504 / X3_SC; then the torch module, until a later refresh."""
        prec = "torch"
        if self.precision == "x3":
            prec = "x3"
            big, vnorm = mha_weight_range(self.encs)
            if not mha_range_ok(big, vnorm):
                import warnings
                warnings.warn(f"x3 rollout encoders: max |w| = {big:.4g} (limit {F16_MAX / X3_SW:.4g}), max row |w_vs|_1 = "
                              f"{vnorm:.4g} (limit {F16_MAX / X3_SC:.4g}): outside the split-f16 range; evaluating in torch")
                prec = "torch"
        self.packed_precision = prec
        if prec == "torch":
            self.packed = [{} for _ in self.encs]
            return
        H, nbw, od = self.H, self.nd * self.K, self.cfg.obstacle_obs_dim
        packed = []
        for enc in self.encs:
            w = pack_mha_tower(enc, H, nbw, od)
            se = enc.self_embed_layer
            if (self.packed_join is None   # (else the join kernel evaluates the self encoder)
                    and self_l2_supported(se) and float(se[2].weight.detach().abs().amax()) < F16_MAX / X3_SW):
                w.update(w_s2p=pack_linear_x3(se[2].weight.detach()), b_s2=se[2].bias.detach().contiguous())
            packed.append(w)
        self.packed = packed
        self._bind_mha()

    def _bind_mha(self):
        if self.packed_precision != "x3" or self.B is None:
            return
        for i, w in enumerate(self.packed):
            t = self.towers[i]
            for name in MHA_TOWER_FIELDS:
                assert w[name].is_contiguous()
                setattr(t, name, w[name].data_ptr())
            t.out = self.out[i].data_ptr()

    def _mha_tokens(self, obs):
        """[T, B, 2H]: both towers' normalised attention tokens (QuadMultiHeadAttentionEncoder.tokens)."""
        if self.packed_precision != "x3":
            return [enc.tokens(obs) for enc in self.encs]
        B = obs.shape[0]
        if self.B != B:
            self.B = B
            self.out = torch.empty(len(self.encs), B, 2 * self.H, dtype=torch.float32, device=obs.device)
            self._bind_mha()
        m = obs.abs().amax()   # layer 0's range check, on the device (read by check_inputs)
        self._obs_absmax = m if self._obs_absmax is None else torch.maximum(self._obs_absmax, m)
        st = ctypes.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        NAT.check(self.L.qs_mha_encoder_x3(ctypes.c_void_p(obs.data_ptr()), obs.shape[1], self.so, self.nd * self.K,
                                           self.cfg.obstacle_obs_dim, B, self.H, self.towers, len(self.encs), st),
                  "qs_mha_encoder_x3")
        return self.out

    def _encode_mha(self, enc, obs, tokens, w):
        se = enc.self_embed_layer
        if "w_s2p" in w:   # the second Linear + Tanh (tanh inputs) as one kernel
            s = linear_tanh_x3(se[1](se[0](obs[:, :self.so])), w["w_s2p"], w["b_s2"])
        else:
            s = se(obs[:, :self.so])
        return enc.feed_forward(torch.cat((s, tokens), dim=1))

    # ---- the MLP family: mean_embed, mlp and no neighbour encoder ----
    def _refresh_enc(self):
        """precision "fp32": the torch modules evaluate this family (it has no fp32-MFMA kernel).  "x3": the kernel,
        unless a weight is outside the split-f16 range (|w| >= 255.9); then the torch modules, until a later refresh."""
        self.packed_precision = "torch"
        self.packed = [{} for _ in self.encs]
        if self.precision != "x3":
            return
        try:
            packed = pack_enc_towers(self.encs)
        except ValueError as e:
            import warnings
            warnings.warn(f"x3 rollout encoders: {e}; evaluating in torch")
            return
        self.packed_precision, self.packed = "x3", packed
        self._bind_enc()

    def _bind_enc(self):
        if self.packed_precision != "x3" or self.B is None:
            return
        for i, w in enumerate(self.packed):
            t = self.towers[i]
            for name, x in w.items():
                assert x.is_contiguous()
                setattr(t, name, x.data_ptr())
            t.out = self.out[i].data_ptr()

    @torch.no_grad()
    def latents(self, obs):
        """[T, B, 2 rnn_size]: both towers' encoder outputs (the feed_forward's), the rows tail() reads -- one launch of
        qs_encoder_mlp_x3 from the raw observations (the tensor is reused by the next call)."""
        assert self.enc and obs.dim() == 2
        if self.packed is None:
            self.refresh()
        if self.packed_precision != "x3":
            return torch.stack([enc(obs) for enc in self.encs])
        assert obs.is_cuda and obs.dtype == torch.float32
        obs = obs.contiguous()
        B = obs.shape[0]
        if self.B != B:
            self.B = B
            self.out = torch.empty(len(self.encs), B, 2 * self.H, dtype=torch.float32, device=obs.device)
            self._bind_enc()
        m = obs.abs().amax()   # layer 0's range check, on the device (read by check_inputs)
        self._obs_absmax = m if self._obs_absmax is None else torch.maximum(self._obs_absmax, m)
        st = ctypes.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        NAT.check(self.L.qs_encoder_mlp_x3(ctypes.c_void_p(obs.data_ptr()), obs.shape[1], self.so,
                                           NAT.ENC_NBR[enc_nbr_kind(self.cfg)], self.K, self.nd,
                                           self.cfg.obstacle_obs_dim, B, self.H, self.towers, len(self.encs), st),
                  "qs_encoder_mlp_x3")
        return self.out

    # ---- the attention families' join: self encoder, obstacle encoder, feed_forward ----
    def _refresh_join(self):
        """Pack both towers for qs_encoder_join_x3.  A weight outside the split-f16 range (|w| >= 255.9), or LayerNorm
        parameters that let a token reach it at the activation scale (sqrt(H) max |ln_g| + max |ln_b| >= 255.9), would
        pack as +-inf: the torch join then evaluates until a later refresh finds everything in range again."""
        import warnings
        self.packed_join = None
        lim = F16_MAX / X3_SX
        if self.mha:
            bound = join_token_bound(self.encs)
            if not bound < lim:   # NaN fails too
                warnings.warn(f"x3 rollout join: token bound sqrt(H) max |ln_g| + max |ln_b| = {bound:.4g} >= {lim:.4g}, "
                              "outside the split-f16 range; evaluating in torch")
                return
        try:
            packed = pack_join_towers(self.encs)
        except ValueError as e:
            warnings.warn(f"x3 rollout join: {e}; evaluating in torch")
            return
        for t, w in zip(self.join_towers, packed):
            for name, x in w.items():
                assert x.is_contiguous()
                setattr(t, name, x.data_ptr())
        self.packed_join = packed

    def join_latents(self, obs, nbr, critic_only=False):
        """[T, B, 2 rnn_size]: the towers' feed_forward outputs from the observations and the neighbour kernels' rows
        nbr[i] ([B, H] pooled, or [B, 2H] tokens), read in place -- one launch of qs_encoder_join_x3 (critic_only: row 1
        alone is computed).  The tensor is reused by the next call."""
        B, T = obs.shape[0], len(self.encs)
        parts = 2 if self.mha else 1
        if self.join_out is None or self.join_out.shape[1] != B or self.join_out.device != obs.device:
            self.join_out = torch.empty(T, B, 2 * self.H, dtype=torch.float32, device=obs.device)
        for i in range(T):
            x = nbr[i]
            assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape == (B, parts * self.H)
            self.join_towers[i].nbr, self.join_towers[i].out = x.data_ptr(), self.join_out[i].data_ptr()
        if self.packed_precision != "x3":   # (else the neighbour kernels' call has taken the layer-0 range statistic)
            m = obs.abs().amax()
            self._obs_absmax = m if self._obs_absmax is None else torch.maximum(self._obs_absmax, m)
        towers, n = (ctypes.pointer(self.join_towers[T - 1]), 1) if critic_only else (self.join_towers, T)
        od = 0 if self.mha else self.cfg.obstacle_obs_dim   # the multi-head family's obstacle values are in its tokens
        st = ctypes.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        NAT.check(self.L.qs_encoder_join_x3(ctypes.c_void_p(obs.data_ptr()), obs.shape[1], self.so, self.so + self.K * self.nd,
                                            od, parts, B, self.H, towers, n, st), "qs_encoder_join_x3")
        return self.join_out

    # ---- the tail: core, decoder, heads, action distribution ----
    def _refresh_tail(self):
        """Pack both towers' chains for qs_policy_tail_x3.  A chain weight outside the split-f16 range (|w| >= 255.9)
        would become +-inf: the torch tail then evaluates until a later refresh finds every weight in range again."""
        pol = self.policy
        chains = (tail_chain(pol.actor_core, pol.actor_decoder), tail_chain(pol.critic_core, pol.critic_decoder))
        heads = (pol.action_net, pol.value_net)
        self.packed_tail = None
        mats = [m.weight for ch in chains for m in ch]
        if mats:
            lim = F16_MAX / X3_SW
            big = float(torch.stack([w.detach().abs().amax() for w in mats]).amax())
            if not big < lim:
                import warnings
                warnings.warn(f"x3 rollout tail: max |w| = {big:.4g} >= {lim:.4g} (f16 range); evaluating in torch")
                return
        pk = pack_mfma_weights_x3(mats) if mats else []
        n = len(chains[0])
        keep = []   # the tensors the towers point into
        for i, (ch, head) in enumerate(zip(chains, heads)):
            t = self.tail_towers[i]
            for l, m in enumerate(ch):
                w, b = pk[i * n + l].contiguous(), m.bias.detach().contiguous()
                t.w_chain[l], t.b_chain[l] = w.data_ptr(), b.data_ptr()
                keep += [w, b]
            w, b = head.weight.detach().contiguous(), head.bias.detach().contiguous()
            assert w.shape == (head.out_features, self.cfg.rnn_size if n else 2 * self.cfg.rnn_size)
            t.w_head, t.b_head, t.n_out = w.data_ptr(), b.data_ptr(), head.out_features
            keep += [w, b]
        ls = pol.log_std.detach().contiguous()
        self.tail_towers[0].log_std = ls.data_ptr()
        self.tail_towers[1].log_std = None
        self.packed_tail = dict(n_layers=n, keep=keep + [ls])

    @torch.no_grad()
    def tail(self, latents_actor, latents_critic, noise=None, deterministic=False):
        """(actions, values [B, 1], log_prob [B]) from the towers' feed_forward outputs [B, 2 rnn_size]: core, decoder,
        action_net / value_net, actions = tanh(mean + exp(log_std) noise) (tanh(mean) when deterministic or without
        noise [B, act_dim]) and their squashed-Gaussian log-prob.  latents_actor None: the critic alone, (None, values,
        None).  tail "x3": one launch of qs_policy_tail_x3, unless refresh() found a chain weight out of range."""
        pol = self.policy
        if self.tail_mode == "x3" and self.packed is None:
            self.refresh()
        if self.tail_mode != "x3" or self.packed_tail is None:
            from .ppo import squashed_log_prob
            values = pol.value_net(pol.critic_decoder(pol.critic_core(latents_critic)))
            if latents_actor is None:
                return None, values, None
            mean = pol.action_net(pol.actor_decoder(pol.actor_core(latents_actor)))
            sample = noise is not None and not deterministic
            actions = torch.tanh(mean + noise * pol.log_std.exp()) if sample else torch.tanh(mean)
            return actions, values, squashed_log_prob(mean, pol.log_std, actions)
        R, dev = self.cfg.rnn_size, latents_critic.device
        B = latents_critic.shape[0]
        lats = [x for x in (latents_actor, latents_critic) if x is not None]
        assert all(x.is_cuda and x.dtype == torch.float32 and x.shape == (B, 2 * R) for x in lats)
        lats = [x.contiguous() for x in lats]
        values = torch.empty(B, 1, dtype=torch.float32, device=dev)
        actions = log_prob = None
        tc = self.tail_towers[1]
        tc.x, tc.out = lats[-1].data_ptr(), values.data_ptr()
        towers, n_towers = self.tail_towers, 2
        if latents_actor is None:
            towers, n_towers = ctypes.pointer(tc), 1
        else:
            actions = torch.empty(B, self.cfg.act_dim, dtype=torch.float32, device=dev)
            log_prob = torch.empty(B, dtype=torch.float32, device=dev)
            ta = self.tail_towers[0]
            if noise is not None and not deterministic:
                assert noise.is_cuda and noise.dtype == torch.float32 and noise.shape == actions.shape
                noise = noise.contiguous()
                ta.eps = noise.data_ptr()
            else:
                ta.eps = None
            ta.deterministic = int(bool(deterministic))
            ta.x, ta.out, ta.log_prob = lats[0].data_ptr(), actions.data_ptr(), log_prob.data_ptr()
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        NAT.check(self.L.qs_policy_tail_x3(B, R, self.packed_tail["n_layers"], towers, n_towers, st), "qs_policy_tail_x3")
        return actions, values, log_prob

    # ---- forward ----
    @torch.no_grad()
    def neighbor_encodings(self, obs):
        """[T, B, H]: both towers' QuadNeighborhoodEncoderAttention outputs (the tensor is reused by the next call)."""
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.dim() == 2
        obs = obs.contiguous()
        B = obs.shape[0]
        if self.packed is None:
            self.refresh()
        if self.mha:   # this family's encodings are its two attention tokens, [T, B, 2H]
            return self._mha_tokens(obs)
        if self.B != B:
            self._alloc(B, obs.device)
        so, H, K = self.so, self.H, self.K
        st = ctypes.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
        x3 = self.packed_precision == "x3"
        if x3:   # the range check of the layer-0 inputs, on the device (read by check_inputs)
            m = obs.abs().amax()
            self._obs_absmax = m if self._obs_absmax is None else torch.maximum(self._obs_absmax, m)
        embed, pool = (self.L.qs_attn_embed_x3, self.L.qs_attn_pool_x3) if x3 else (self.L.qs_attn_embed, self.L.qs_attn_pool)
        NAT.check(embed(ctypes.c_void_p(obs.data_ptr()), obs.shape[1], so, so, B, K, self.nd, H,
                        self.towers, len(self.encs), st), "qs_attn_embed")
        for i, w in enumerate(self.packed):
            if "w_a1mp" in w:
                linear_bias_x3(self.e_mean[i], w["w_a1mp"], w["b_a1"], out=self.P[i])
            else:
                torch.addmm(w["b_a1"], self.e_mean[i], w["w_a1m"].t(), out=self.P[i])
        NAT.check(pool(B, K, H, self.towers, len(self.encs), st), "qs_attn_pool")
        return self.out

    def _encode(self, enc, obs, nbr_out, w=None):
        if self.mha:
            return self._encode_mha(enc, obs, nbr_out, w)
        so, na = self.so, enc.all_neighbor_obs_size
        se = enc.self_encoder
        if w is not None and "w_s2p" in w:   # x3: the second Linear + Tanh (tanh inputs) as one kernel
            parts = [linear_tanh_x3(se[1](se[0](obs[:, :so])), w["w_s2p"], w["b_s2"]), nbr_out]
        else:
            parts = [se(obs[:, :so]), nbr_out]
        if enc.obstacle_encoder is not None:
            parts.append(enc.obstacle_encoder(obs[:, so + na:]))
        if w is not None and "w_ffp" in w and cat_free(parts):   # x3, [self | neighbour] read in place
            return linear_tanh_cat_x3(parts[0], parts[1], w["w_ffp"], w["b_ff"])
        x = torch.cat(parts, dim=1)
        if w is not None and "w_ffp" in w:   # x3: the feed_forward's Linear + Tanh as one kernel (|x| <= 1: tanh rows)
            return linear_tanh_x3(x, w["w_ffp"], w["b_ff"])
        return enc.feed_forward(x)

    @torch.no_grad()
    def forward(self, obs, deterministic=False):
        """SwarmActorCritic.forward: (actions, values [B, 1], log_prob [B])."""
        from .ppo import squashed_log_prob
        pol = self.policy
        if self.enc:   # tail(): one launch, or the torch row (the same draw as randn_like(mean) below)
            lat = self.latents(obs)
            noise = None if deterministic else torch.randn((obs.shape[0], self.cfg.act_dim), device=obs.device)
            return self.tail(lat[0], lat[1], noise, deterministic)
        nbr = self.neighbor_encodings(obs)
        if self.join_mode == "x3" and self.packed_join is not None:   # neighbour kernels, join, tail(): no torch GEMM
            lat = self.join_latents(obs.contiguous(), nbr)
            noise = None if deterministic else torch.randn((obs.shape[0], self.cfg.act_dim), device=obs.device)
            return self.tail(lat[0], lat[1], noise, deterministic)
        if self.tail_mode == "x3":
            lat = [self._encode(enc, obs, nbr[i], self.packed[i]) for i, enc in enumerate(self.encs)]
            # (the draw of randn_like(mean) below: same generator, same shape)
            noise = None if deterministic else torch.randn((obs.shape[0], self.cfg.act_dim), device=obs.device)
            return self.tail(lat[0], lat[1], noise, deterministic)
        a_lat = pol.actor_decoder(pol.actor_core(self._encode(pol.actor_encoder, obs, nbr[0], self.packed[0])))
        mean = pol.action_net(a_lat)
        values = pol.value_net(pol.critic_decoder(pol.critic_core(self._encode(pol.critic_encoder, obs, nbr[1],
                                                                               self.packed[1]))))
        if deterministic:
            actions = torch.tanh(mean)
        else:
            actions = torch.tanh(mean + torch.randn_like(mean) * pol.log_std.exp())
        return actions, values, squashed_log_prob(mean, pol.log_std, actions)

    __call__ = forward

    @torch.no_grad()
    def predict_values(self, obs):
        pol = self.policy
        if self.enc:
            return self.tail(None, self.latents(obs)[1])[1]
        nbr = self.neighbor_encodings(obs)
        if self.join_mode == "x3" and self.packed_join is not None:
            return self.tail(None, self.join_latents(obs.contiguous(), nbr, critic_only=True)[1])[1]
        if self.tail_mode == "x3":
            return self.tail(None, self._encode(pol.critic_encoder, obs, nbr[1], self.packed[1]))[1]
        return pol.value_net(pol.critic_decoder(pol.critic_core(self._encode(pol.critic_encoder, obs, nbr[1],
                                                                             self.packed[1]))))
