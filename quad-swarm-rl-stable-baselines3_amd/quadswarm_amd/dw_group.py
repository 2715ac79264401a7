"""The x3 update's weight gradients as one grouped launch per autograd node (csrc/qs_dw_group.h, qs_dw_group_x3).

plan_encoder / plan_tail turn a policy into the node's ordered job list -- which pre-activation gradient pairs with which
save or observation columns, and which block of which parameter's gradient the product is (pure Python: no device).
Group binds a plan to a runner's buffers as a qs_dw_job table and launches it: FusedEncoderTrain(policy, dw="grouped"),
FusedTailTrain(policy, dw="grouped"), PPOTrainer(update_dw="grouped"); tests/test_dw_group_cpu.py, test_gpu_dw_group.py.

The job table lives in host memory (a ctypes array) and travels in the kernel arguments, so no device copy, torch launch or
synchronisation carries it.  The runners reuse their buffers, so G, the saves and colmax are bound once per minibatch size
(Group.bind); what changes per minibatch -- the observation / latent rows a job reads as A and the fresh gradient tensors
it writes -- is rewritten into the table before every launch (Group.run)."""
import collections
import ctypes

import torch

from . import _native as NAT
from .policy_fused import enc_nbr_kind

# g / a: buffer names of the job's tower (a "obs" / "lat": the node's input rows, bound per call); g_col / a_col: the first
# column of the slice; rows: "B" or "BK"; cm: the tower's colmax row; dst, (r0, c0): the index in the node's params() of
# the weight and the block's corner; db: the index of the bias whose H entries from db_off the job's column sums are
Job = collections.namedtuple("Job", "tower g g_col a a_col a_cols kind a_rows_per a_inner rows cm dst r0 c0 db db_off")

WS_CAP = 256 << 20   # bytes of workspace a group may take: bounds `parts` at large H x jobs
STEP = 16            # rows per step (qs_dw_group.h DG_STEP)


def plan_encoder(policy):
    """The jobs of FusedEncoderTrain's node in params() order, both towers: per tower the self encoder's two layers, the
    neighbour encoder's (mlp 3, mean_embed 2, none 0), the obstacle encoder's 2, then the feed_forward's 2 NP blocks."""
    from .enc_mlp_train import CM_FF, CM_N1, CM_N2, CM_N3, CM_O1, CM_O2, CM_S1, CM_S2, tower_params
    c = policy.cfg
    H, K, nd, so, od = c.rnn_size, c.num_use_neighbor_obs, c.neighbor_obs_dim, c.self_obs_dim, c.obstacle_obs_dim
    kind = enc_nbr_kind(c)
    jobs, base = [], 0
    for t, enc in enumerate((policy.actor_encoder, policy.critic_encoder)):
        # (kind, g, a: the save, or the first obs column, a_cols, cm, rows, a_rows_per, a_inner) per layer, params() order
        layers = [("obs", "dpre_s1", 0, so, CM_S1, "B", 1, 0), ("tanh", "dpre_s2", "s1", H, CM_S2, "B", 1, 0)]
        parts = ["s2"]
        if kind == "mlp":
            layers += [("obs", "dpre_n1", so, K * nd, CM_N1, "B", 1, 0), ("tanh", "dpre_n2", "n1", H, CM_N2, "B", 1, 0),
                       ("tanh", "dpre_n3", "n2", H, CM_N3, "B", 1, 0)]
            parts.append("n3")
        elif kind == "mean":   # rows q K + k: neighbour k of agent q
            layers += [("obs", "dpre_n1", so, nd, CM_N1, "BK", K, nd), ("tanh", "dpre_n2", "n1", H, CM_N2, "BK", 1, 0)]
            parts.append("m")
        if od:
            layers += [("obs", "dpre_o1", so + K * nd, od, CM_O1, "B", 1, 0), ("tanh", "dpre_o2", "o1", H, CM_O2, "B", 1, 0)]
            parts.append("o2")
        for i, (kd, g, a, cols, cm, rows, per, inner) in enumerate(layers):
            k, obs = base + 2 * i, kd == "obs"
            jobs.append(Job(t, g, 0, "obs" if obs else a, a if obs else 0, cols, kd, per, inner, rows, cm, k, 0, 0, k + 1, 0))
        k = base + 2 * len(layers)
        for z in range(2):   # the [2H, NP H] feed_forward weight by blocks; the bias half with the first block
            for p, a in enumerate(parts):
                jobs.append(Job(t, "dpre_ff", z * H, a, 0, H, "tanh", 1, 0, "B", CM_FF + z, k, z * H, p * H,
                                k + 1 if p == 0 else None, z * H))
        base += len(tower_params(enc))
        assert k + 2 == base
    return jobs


def plan_tail(policy):
    """The jobs of FusedTailTrain's node, both towers: per chain layer one job, layer 0 ([R, 2R]) as two column blocks against
    the latents' halves.  The heads' and log_std's gradients are not jobs (sums of the backward's per-block parts)."""
    from .policy_fused import tail_chain
    R = policy.cfg.rnn_size
    jobs, base = [], 0
    for t, ch in enumerate((tail_chain(policy.actor_core, policy.actor_decoder),
                            tail_chain(policy.critic_core, policy.critic_decoder))):
        for l in range(len(ch)):
            k = base + 2 * l
            if l == 0:
                jobs += [Job(t, "dpre0", 0, "lat", h * R, R, "tanh", 1, 0, "B", 0, k, 0, h * R, k + 1 if h == 0 else None, 0)
                         for h in range(2)]
            else:
                jobs.append(Job(t, f"dpre{l}", 0, f"y{l - 1}", 0, R, "tanh", 1, 0, "B", l, k, 0, 0, k + 1, 0))
        base += 2 * len(ch) + 2   # the head's weight and bias follow the chain's
    return jobs


def choose_parts(n_jobs, H, max_rows, cus):
    """Row parts per job: enough that jobs x parts fills the device about once, more when the longest job would walk over
    64 steps a part, within the workspace cap and the job's steps."""
    steps = (max_rows + STEP - 1) // STEP
    parts = max(cus // n_jobs, (steps + 63) // 64, 1)
    cap = max(1, WS_CAP // (n_jobs * (H * H + H) * 4))
    return max(1, min(parts, cap, steps))


class Group:
    """A plan bound to one node's buffers.  params: the node's params() (shapes of the gradients to return)."""

    def __init__(self, plan, params, H):
        if not 1 <= len(plan) <= NAT.DW_GROUP_MAX_JOBS:
            raise ValueError(f"a weight-gradient group holds 1..{NAT.DW_GROUP_MAX_JOBS} jobs")
        self.plan, self.H = plan, H
        self.shapes = [tuple(p.shape) for p in params]
        self.covered = sorted({j.dst for j in plan} | {j.db for j in plan if j.db is not None})
        self.jobs = (NAT.QsDwJob * len(plan))()
        self.L = NAT.lib()
        self.ws = None

    def bind(self, bufs, colmax, B, K, dev):
        """What stays for a minibatch size: bufs[tower][name] the runner's tensors, colmax[tower] [n, grid_x, H]."""
        H = self.H
        rows = {"B": B, "BK": B * K}
        for q, j in zip(self.jobs, self.plan):
            G = bufs[j.tower][j.g]
            q.G, q.ldg, q.R = G.data_ptr() + 4 * j.g_col, G.stride(0), rows[j.rows]
            cm = colmax[j.tower][j.cm]
            assert cm.is_contiguous() and cm.shape[1] == H
            q.colmax, q.colmax_n = cm.data_ptr(), cm.shape[0]
            q.a_cols, q.a_kind = j.a_cols, NAT.DW_A_TANH if j.kind == "tanh" else NAT.DW_A_OBS
            q.a_rows_per, q.a_inner = j.a_rows_per, j.a_inner
            q.ldw = self.shapes[j.dst][1]
            if j.a in bufs[j.tower]:
                A = bufs[j.tower][j.a]
                q.A, q.lda = A.data_ptr() + 4 * j.a_col, A.stride(0)
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        self.parts = choose_parts(len(self.plan), H, max(rows[j.rows] for j in self.plan), cus)
        n = ctypes.c_size_t()
        NAT.check(self.L.qs_dw_group_workspace(len(self.plan), H, self.parts, ctypes.byref(n)), "qs_dw_group_workspace")
        self.ws = torch.empty(n.value // 4, dtype=torch.float32, device=dev)

    def run(self, inputs, dev):
        """One group call.  inputs[tower][name]: this minibatch's input rows ("obs" / "lat").  Returns the node's gradients
        in params() order as fresh tensors, None where no job writes (the caller's)."""
        out = [None] * len(self.shapes)
        for k in self.covered:
            out[k] = torch.empty(self.shapes[k], dtype=torch.float32, device=dev)
        for q, j in zip(self.jobs, self.plan):
            if j.a in inputs[j.tower]:
                A = inputs[j.tower][j.a]
                q.A, q.lda = A.data_ptr() + 4 * j.a_col, A.stride(0)
            q.dW = out[j.dst].data_ptr() + 4 * (j.r0 * q.ldw + j.c0)
            q.db = out[j.db].data_ptr() + 4 * j.db_off if j.db is not None else None
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        NAT.check(self.L.qs_dw_group_x3(self.jobs, len(self.plan), self.H, self.parts, ctypes.c_void_p(self.ws.data_ptr()),
                                        self.ws.numel() * 4, st), "qs_dw_group_x3")
        return out
