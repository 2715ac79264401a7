"""Flavor B's neighbour observation types restated in numpy (get_rel_pos_vel_item quadrotor_multi.py:275-319,
neighborhood_indices :344-375, the extend_obs_space clip quadrotor_single.py:280-326) and the comparison the GPU
tests use.  Test infrastructure: pinned to the reference by tests/golden/neighbors_variants*.npz
(test_neighbor_variants_cpu.py)."""
import numpy as np

from parity_utils import _one_to_one

DIM = {"pos_vel": 6, "pos": 3, "npos": 3, "pos_Rz": 6, "pos_vel_Rz": 9, "pos_vel_R": 15, "rng3": 3}
DETERMINISTIC = ("pos", "npos", "pos_Rz", "pos_vel_Rz", "pos_vel_R")
# neighbors_variants*.npz: the file that holds a type's recorded blocks (tools/gen_golden_nbr.py file_of)
EXCUSES = {"rows": 0, "compared": 0}


def golden_file(ntype, n):
    if ntype in ("pos", "npos"):
        return "neighbors_variants"
    return f"neighbors_variants_{ntype}_n{'32' if n > 8 else '8'}" if ntype == "pos_vel_R" else f"neighbors_variants_{ntype}"


def packed_rows(ntype, pos, vel, rot, i):
    """get_rel_pos_vel_item of drone i against every j (row i is the drone itself): rel pos, rel vel, then
    rot[i].T @ rot[j][:, 2] (Rz) or rot[i].T @ rot[j] flattened row-major (R).  "Rz" is tested before "R" and
    "npos" (whose noise the reference discards) is "pos"."""
    parts = [pos - pos[i]]
    if "vel" in ntype:
        parts.append(vel - vel[i])
    if "Rz" in ntype:
        parts.append(np.einsum("ca,jc->ja", rot[i], rot[:, :, 2]))
    elif "R" in ntype:
        parts.append(np.einsum("ca,jcb->jab", rot[i], rot).reshape(len(pos), 9))
    return np.concatenate(parts, 1)


def neighbor_block(ntype, pos, vel, rot, i, K, room_range, dtype=np.float64):
    """(keys [N], clipped rows [N, d], slot order [K]) of drone i.  Key: the norm of the whole packed row clamped
    below at 0.01 (the drone itself: inf); K < N - 1 sorts by it (stable), K == N - 1 keeps index order.
    dtype float32: the arithmetic of an fp32 implementation -- the varying part of the squared key summed in fp32
    (the constant 3 of an R block / 1 of an Rz block left out, clamp 1e-4 where there is no such block)."""
    pos, vel, rot = (np.asarray(x, dtype=dtype) for x in (pos, vel, rot))
    N = len(pos)
    row = packed_rows(ntype, pos, vel, rot, i)
    if dtype == np.float64:
        keys = np.maximum(np.linalg.norm(row, axis=1), 0.01)
    else:
        nv = 6 if "vel" in ntype else 3
        const = 1.0 if "Rz" in ntype else (3.0 if "R" in ntype else 0.0)
        s = np.zeros(N, dtype)
        for c in range(nv):
            s = s + row[:, c] * row[:, c]
        keys = np.sqrt(np.maximum(s, dtype(0.0 if const else 1e-4)).astype(np.float64) + const)
        order_key = np.maximum(s, dtype(0.0 if const else 1e-4))
    keys = keys.astype(np.float64)
    keys[i] = np.inf
    lo = np.concatenate([np.full(3, float(room_range)), np.full(3, 6.0) if "vel" in ntype else np.zeros(0),
                         np.ones(row.shape[1] - (6 if "vel" in ntype else 3))])
    rows = np.clip(row, -lo, lo)
    if K == N - 1:
        order = [j for j in range(N) if j != i]
    else:
        sk = keys if dtype == np.float64 else np.where(np.arange(N) == i, np.inf, order_key)
        order = [int(j) for j in np.argsort(sk, kind="stable")[:K]]
    return keys, rows, order


def blocks(ntype, pos, vel, rot, N, K, room_range, dtype=np.float64):
    """The neighbour blocks [I, K d] of drones laid out env-major (pos, vel [I, 3], rot [I, 3, 3])."""
    out = np.zeros((len(pos), K * DIM[ntype]))
    for e in range(len(pos) // N):
        sl = slice(e * N, (e + 1) * N)
        for i in range(N):
            _, rows, order = neighbor_block(ntype, pos[sl], vel[sl], rot[sl], i, K, room_range, dtype)
            out[e * N + i] = rows[order].reshape(-1)
    return out


def selection_diffs(ntype, pos, vel, rot, N, K, room_range):
    """Rows whose fp32 selection (slot order) differs from the fp64 one: what an exact fp32 implementation
    would need excused on these states."""
    n = 0
    for e in range(len(pos) // N):
        sl = slice(e * N, (e + 1) * N)
        for i in range(N):
            o64 = neighbor_block(ntype, pos[sl], vel[sl], rot[sl], i, K, room_range)[2]
            o32 = neighbor_block(ntype, pos[sl], vel[sl], rot[sl], i, K, room_range, np.float32)[2]
            n += o64 != o32
    return n


def assert_nbr_match(got, ntype, pos, vel, rot, N, K, room_range, atol=2e-4, rtol=1e-4, key_tol=1e-4, max_excused=None,
                     rows=None):
    """got [I, K d] against the restatement of (pos, vel [I, 3], rot [I, 3, 3]), slot-exact.  A block that differs is
    accepted only through a one-to-one mapping of its slots onto distinct neighbours in which every slot whose
    neighbour is not the restatement's holds one whose key ties with it within key_tol relative + 1e-5.  Excused
    rows are counted and capped at 1 % of the rows, at least 2.  rows: a mask of the rows to compare."""
    got = np.asarray(got, dtype=np.float64)
    d = DIM[ntype]
    excused = 0
    idx = range(len(got)) if rows is None else np.flatnonzero(rows)
    for r in idx:
        e, i = divmod(int(r), N)
        sl = slice(e * N, (e + 1) * N)
        keys, relc, order = neighbor_block(ntype, pos[sl], vel[sl], rot[sl], i, K, room_range)
        g = got[r].reshape(K, d)
        if np.isclose(g, relc[order], atol=atol, rtol=rtol).all():
            continue
        cands = []
        for s in range(K):
            tol = atol + rtol * np.abs(g[s])
            ok = [j for j in range(N) if j != i and np.all(np.abs(relc[j] - g[s]) <= tol)]
            assert ok, f"row {r} slot {s}: no neighbour of drone {i} matches {g[s]} (want {relc[order[s]]})"
            cands.append(ok)
        m = _one_to_one(cands)
        assert m is not None, f"row {r}: the slots do not hold {K} distinct neighbours ({cands})"
        for s in range(K):
            j, w = m[s], order[s]
            if j != w:
                assert abs(keys[j] - keys[w]) <= key_tol * max(keys[j], keys[w]) + 1e-5, \
                    f"row {r} slot {s}: neighbour {j} (key {keys[j]:.9g}) where the reference's sort puts {w} (key {keys[w]:.9g})"
        excused += 1
    EXCUSES["rows"] += excused
    EXCUSES["compared"] += len(idx)
    limit = max(2, len(idx) // 100) if max_excused is None else max_excused
    assert excused <= limit, f"{excused} rows excused by sort-key ties (limit {limit})"
    return excused
