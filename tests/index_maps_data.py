"""Seeded cases and plain numpy oracles of the integer index-map kernels (test helper, not a test module):
csrc/rows_pack.hip - mhr_seq_pack_maps, mhr_seq_pack_maps_guarded, mhr_rows_gather_masked; csrc/tokens.hip - mhr_token_compact,
mhr_row_maps, mhr_nce_log_counters.  Every oracle restates the contract of include/mhr.h in a few numpy lines; nothing here needs
a GPU or imports the project.  tests/test_cpu_index_maps.py checks each oracle against a second formulation and the cases against
the conditions they are meant to meet; tests/test_gpu_index_maps.py compares the kernels with the oracles, bit for bit."""
import numpy as np

SENTINEL = 0x5A5A5A5A                    # fill of int32 outputs whose contract says "untouched"
LIVE_BYTES = (1, 2, 0x80, 0xFF)          # any nonzero mask byte is live
CHUNK = 4096                             # slots / tokens per workgroup of the two-launch scans in csrc/tokens.hip


# ----------------------------------------------------------------------------------------------------------------------
# oracles
# ----------------------------------------------------------------------------------------------------------------------
def pack_maps_oracle(valid, cap):
    """valid [B, L] (nonzero = valid), cap -> (cu_rows [B + 1], src_of [cap], row_of [B L], overflow): the valid positions numbered
    sequence by sequence in window order, those past the capacity dropped."""
    v = np.asarray(valid) != 0
    flat = np.flatnonzero(v.reshape(-1))
    total = int(flat.size)
    cu = np.concatenate(([0], np.minimum(np.cumsum(v.sum(axis=1)), cap))).astype(np.int32)
    kept = flat[:cap]
    src_of = np.full(cap, -1, dtype=np.int32)
    src_of[:kept.size] = kept
    row_of = np.full(v.size, -1, dtype=np.int32)
    row_of[kept] = np.arange(kept.size)
    return cu, src_of, row_of, (total if total > cap else 0)


def guard_oracle(guard, total, cap):
    """The sticky overflow record after one more call: (overflowing calls, largest count seen, the capacity of the call that set
    it, 0); a fitting call changes nothing."""
    g = list(guard)
    if total > cap:
        g[0] += 1
        if g[1] < total:
            g[1], g[2] = total, cap
    return g


def gather_masked_oracle(src, idx):
    """out[r] = src[idx[r]] where idx[r] >= 0, zeros elsewhere (src [n, dim] of any numpy dtype: the tests pass bit patterns)."""
    idx = np.asarray(idx)
    out = np.zeros((idx.size, src.shape[1]), dtype=src.dtype)
    out[idx >= 0] = src[idx[idx >= 0]]
    return out


def compact_oracle(mask, q_all, p_all, o_all, tok_cap, packed=None):
    """mask [G, n_slots] (nonzero = live), q_all [G, n_slots], p_all / o_all [n_slots], tok_cap -> dict of
      slots / q / p / o : per group, the ascending live slots cut at tok_cap and their table values,
      n_tok [G] = min(live, tok_cap),  tok_of_slot [G, n_slots] (-1: dead, or live at list position >= tok_cap),
      bad : with packed = (row_of, L, H, head_stride) the listed slots without a packed row (row < 0 or >= head_stride); their
            q is row 0 of the head.  q is then h * head_stride + row_of[b L + l] of the window form q_all = (b H + h) L + l."""
    mask = np.asarray(mask)
    G, n_slots = mask.shape
    res = dict(slots=[], q=[], p=[], o=[], n_tok=np.zeros(G, dtype=np.int32),
               tok_of_slot=np.full((G, n_slots), -1, dtype=np.int32), bad=0)
    for g in range(G):
        s = np.flatnonzero(mask[g] != 0)[:tok_cap]
        q = np.asarray(q_all)[g, s].astype(np.int64)
        if packed is not None:
            row_of, L, H, head_stride = packed
            b, rem = np.divmod(q, H * L)
            h, l = np.divmod(rem, L)
            r = np.asarray(row_of)[b * L + l].astype(np.int64)
            lost = (r < 0) | (r >= head_stride)
            res["bad"] += int(lost.sum())
            q = h * head_stride + np.where(lost, 0, r)
        res["slots"].append(s)
        res["q"].append(q.astype(np.int32))
        res["p"].append(np.asarray(p_all)[s].astype(np.int32))
        res["o"].append(np.asarray(o_all)[s].astype(np.int32))
        res["n_tok"][g] = s.size
        res["tok_of_slot"][g, s] = np.arange(s.size)
    return res


def row_maps_oracle(q):
    """q = q_idx[:n_tok] of one group -> (row_q [n_row], row_first [n_row + 1], tok2row [n_tok], n_row): a row is a run of
    consecutive tokens with one query row; row_first[n_row] = n_tok.  (By contract tok2row[t >= n_tok] = 0 and the entries of
    row_q / row_first behind these are untouched.)"""
    q = np.asarray(q)
    n_tok = q.size
    heads = np.concatenate(([True], q[1:] != q[:-1]))[:n_tok]
    first = np.flatnonzero(heads)
    return (q[first].astype(np.int32), np.concatenate((first, [n_tok])).astype(np.int32),
            (np.cumsum(heads) - 1).astype(np.int32), int(first.size))


def log_counters_oracle(n_valid, rank, o_idx, n_tok, group, ks):
    """[G, cap] token tables, n_tok [G] -> f32 [1 + len(ks)]: mean n_valid and mean(rank < k) over the tokens t < n_tok[group]
    with o_idx == 0.  Integer sums in Python ints; one fp64 division rounded once to f32, which is the kernel's arithmetic."""
    n = int(n_tok[group])
    sel = np.flatnonzero(np.asarray(o_idx)[group, :n] == 0)
    cnt = int(sel.size)
    sums = [sum(int(v) for v in np.asarray(n_valid)[group, sel])]
    sums += [int((np.asarray(rank)[group, sel] < k).sum()) for k in ks]
    return np.array([np.float32(np.float64(v) / np.float64(max(cnt, 1))) for v in sums], dtype=np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# mhr_seq_pack_maps: shapes x masks, and the capacities of a mask
# ----------------------------------------------------------------------------------------------------------------------
# (256, 3) / (257, 3): both sides of one sequence per scan thread; (1000, 7): four per thread, the last threads own none
PACK_SHAPES = [(1, 1), (3, 64), (3, 65), (2, 129), (4, 200), (256, 3), (257, 3), (1000, 7)]
PACK_MASKS = ["mixed", "empty", "full", "bytes"]


def pack_mask(B, L, kind):
    """[B, L] uint8.  mixed: density 0.6 with sequence 0 empty and sequence 1 full (B >= 2); bytes: the same, the valid bytes drawn
    from LIVE_BYTES."""
    rng = np.random.default_rng(1000 * B + L)
    if kind == "empty":
        return np.zeros((B, L), dtype=np.uint8)
    if kind == "full":
        return np.ones((B, L), dtype=np.uint8)
    v = rng.random((B, L)) < 0.6
    if B >= 2:
        v[0], v[1] = False, True
    else:
        v[0, 0] = True
    if kind == "bytes":
        return np.where(v, rng.choice(np.array(LIVE_BYTES, dtype=np.uint8), size=(B, L)), 0).astype(np.uint8)
    return v.astype(np.uint8)


def pack_caps(valid):
    """[(name, capacity, overflows)] of a mask: the exact count, one and 3000 rows of slack (the tail clear of src_of then runs more
    than one pass of its 16 x 64 lanes), and the overflowing ones - one row short, a cut in the middle of a sequence, a cut exactly
    between two sequences, capacity 1.  Capacities below 1 (not accepted) and repeats are left out."""
    lens = (np.asarray(valid) != 0).sum(axis=1)
    cu = np.concatenate(([0], np.cumsum(lens)))
    total = int(cu[-1])
    caps = [("exact", total, False), ("slack1", total + 1, False), ("slack3000", total + 3000, False), ("short1", total - 1, True)]
    mid = [int(cu[b] + lens[b] // 2) for b in range(len(lens)) if lens[b] >= 2]
    if mid:
        caps.append(("mid", mid[len(mid) // 2], True))
    edge = [int(c) for c in cu[1:-1] if 0 < c < total]
    if edge:
        caps.append(("edge", edge[len(edge) // 2], True))
    caps.append(("one", 1, total > 1))
    out, seen = [], set()
    for name, cap, over in caps:
        if cap >= 1 and cap not in seen:
            seen.add(cap)
            out.append((name, cap, over))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# mhr_rows_gather_masked
# ----------------------------------------------------------------------------------------------------------------------
GATHER_DIMS = {"f32": [4, 64, 256, 260, 520], "bf16": [8, 64, 512, 520, 1032]}    # a wave covers 1024 bytes of a row per pass
GATHER_N_OUT = [1, 3, 4, 5]                    # around the 4 rows a wave keeps in flight
GATHER_N_OUT_LONG = 131072 + 5                 # more than one pass of the 8192-workgroup grid (16 rows per workgroup)
GATHER_PATTERNS = ["none", "all", "mixed", "dup"]
GATHER_N_SRC = 37


def gather_idx(n_out, n_src, pattern):
    """int32 [n_out].  none: every row dropped (-1); all: every row read; mixed: about a third dropped; dup: three source rows
    read over and over (the unpack direction)."""
    rng = np.random.default_rng(n_out * 7 + len(pattern))
    if pattern == "none":
        return np.full(n_out, -1, dtype=np.int32)
    if pattern == "dup":
        return rng.choice(np.array([0, n_src // 2, n_src - 1]), size=n_out).astype(np.int32)
    idx = rng.integers(0, n_src, size=n_out).astype(np.int32)
    if pattern == "mixed":
        idx[rng.random(n_out) < 0.35] = -1
        idx[0] = -1 if n_out > 1 else idx[0]
    return idx


# ----------------------------------------------------------------------------------------------------------------------
# mhr_token_compact
# ----------------------------------------------------------------------------------------------------------------------
# (2, 4136): group 1 starts 8 bytes off a 16-byte boundary, so the count kernel takes its vector path for group 0 and its
# scalar path for group 1 in one call; 66 chunks: the stride-64 loop over the chunk counts iterates
COMPACT_SHAPES = [(1, 1), (2, 15), (2, 16), (2, 4095), (3, 4096), (2, 4097), (2, 4136), (1, 66 * CHUNK + 40)]
COMPACT_MASKS = ["dead", "live", "sparse", "edges"]
COMPACT_BYTES_SHAPES = [(2, 4136), (3, 4096)]
# a token capacity below the live count of every group (the edges mask has two live slots per chunk boundary: 66 chunks only)
COMPACT_CUT = [(G, n, kind, cap) for (G, n, kinds) in [(2, 4136, ("sparse", "live")), (3, 4096, ("sparse", "live")),
                                                      (1, 66 * CHUNK + 40, ("sparse", "live", "edges"))]
               for kind in kinds for cap in (32, 64)]


def compact_mask(G, n_slots, kind):
    """[G, n_slots] uint8.  dead / live: density 0 / 1; sparse: density 0.3; edges: live only in the last slot of every chunk and
    the first slot of the next; bytes: sparse, the live bytes drawn from LIVE_BYTES."""
    rng = np.random.default_rng(G * 100003 + n_slots)
    if kind == "dead":
        return np.zeros((G, n_slots), dtype=np.uint8)
    if kind == "live":
        return np.ones((G, n_slots), dtype=np.uint8)
    if kind == "edges":
        s = np.arange(n_slots)
        one = ((s % CHUNK == CHUNK - 1) | ((s % CHUNK == 0) & (s > 0))).astype(np.uint8)
        return np.repeat(one[None], G, axis=0)
    v = rng.random((G, n_slots)) < 0.3
    if kind == "bytes":
        return np.where(v, rng.choice(np.array(LIVE_BYTES, dtype=np.uint8), size=(G, n_slots)), 0).astype(np.uint8)
    assert kind == "sparse"
    return v.astype(np.uint8)


def compact_tables(G, n_slots):
    """(q_all [G, n_slots], p_all [n_slots], o_all [n_slots]) int32."""
    rng = np.random.default_rng(n_slots + 17 * G)
    return (rng.integers(0, 1 << 20, size=(G, n_slots)).astype(np.int32), rng.integers(0, 1 << 20, size=n_slots).astype(np.int32),
            rng.integers(0, 8, size=n_slots).astype(np.int32))


# packed head rows: B windows of L positions, H heads, one slot per (b, h, l) in a shuffled order; the row map is made at a
# capacity PACKED_DROP rows below the valid count, and the live slots ignore the validity mask - so live tokens without a packed
# row exist for both reasons
PACKED_B, PACKED_L, PACKED_H, PACKED_G, PACKED_DROP, PACKED_STRIDE_PAD = 8, 40, 3, 2, 20, 5
PACKED_TOK_CAPS = [None, 64]


def packed_case():
    """-> (valid [B, L] uint8, capacity, mask [G, n_slots] uint8, q_all [G, n_slots], p_all, o_all)."""
    rng = np.random.default_rng(77)
    B, L, H, G = PACKED_B, PACKED_L, PACKED_H, PACKED_G
    valid = (rng.random((B, L)) < 0.7).astype(np.uint8)
    n_slots = B * H * L
    q_all = np.stack([rng.permutation(n_slots) for _ in range(G)]).astype(np.int32)
    mask = (rng.random((G, n_slots)) < 0.5).astype(np.uint8)
    _, p_all, o_all = compact_tables(G, n_slots)
    return valid, int(valid.sum()) - PACKED_DROP, mask, q_all, p_all, o_all


# ----------------------------------------------------------------------------------------------------------------------
# mhr_row_maps
# ----------------------------------------------------------------------------------------------------------------------
ROW_G = 3
ROW_TOK_CAPS = [32, 4096, 4128, 8192 + 32, 66 * CHUNK + 32]
ROW_N_TOK = [0, 1, 15, 16, 17, 4095, 4096, 4097]            # ... and the capacity itself
ROW_PATTERNS = ["own", "single", "runs", "straddle", "starts", "aaba"]


def row_cap_of(tok_cap):
    return tok_cap + 32                                       # the product's row capacity (ops.nce_fwd)


def row_query(n_tok, pattern, rng):
    """int32 [n_tok] query rows.  own: every token its own row; single: one run; runs: random run lengths 1 .. 8 (prediction
    offsets sharing a position); straddle: runs, and one run across every chunk boundary 4096 k - 1 | 4096 k; starts: a run starts
    exactly at every chunk boundary and at half of the 16-token thread boundaries; aaba: two values taking turns, so equal values sit
    in runs that are not adjacent."""
    t = np.arange(n_tok)
    if pattern == "own":
        heads = np.ones(n_tok, dtype=bool)
    elif pattern == "single":
        heads = np.zeros(n_tok, dtype=bool)
    elif pattern in ("runs", "straddle", "aaba"):
        heads = np.zeros(n_tok, dtype=bool)
        starts = np.cumsum(rng.integers(1, 4 if pattern == "aaba" else 9, size=n_tok + 1))
        heads[starts[starts < n_tok]] = True
        if pattern == "straddle":
            heads[((t + 5) % CHUNK <= 10) & (t >= CHUNK - 5)] = False
    else:
        assert pattern == "starts"
        heads = rng.random(n_tok) < 0.15
        heads[(t % 16 == 0) & (rng.random(n_tok) < 0.5)] = True
        heads[t % CHUNK == 0] = True
    run = np.cumsum(heads)
    if pattern == "aaba":
        return np.where(run % 2 == 0, 3, 9).astype(np.int32)
    return (11 + 3 * run).astype(np.int32)


def row_cases(tok_cap):
    """[(pattern, n_tok [G], q_idx [G, tok_cap])]: every live count of ROW_N_TOK that fits (and tok_cap itself) under every pattern,
    three groups to a call.  Behind n_tok the list repeats its last live value in the even groups and holds random rows in the
    odd ones: nothing there may show in the maps."""
    counts = [n for n in ROW_N_TOK if n <= tok_cap]
    counts += [tok_cap] if tok_cap not in counts else []
    counts += counts[:(-len(counts)) % ROW_G]
    out = []
    for pi, pattern in enumerate(ROW_PATTERNS):
        rng = np.random.default_rng(tok_cap * 31 + pi)
        order = counts[pi % len(counts):] + counts[:pi % len(counts)]    # a count meets every group position over the patterns
        for c0 in range(0, len(order), ROW_G):
            n_tok = np.array(order[c0:c0 + ROW_G], dtype=np.int32)
            q_idx = np.empty((ROW_G, tok_cap), dtype=np.int32)
            for g, n in enumerate(n_tok):
                q_idx[g, :n] = row_query(int(n), pattern, rng)
                if g % 2 == 0:
                    q_idx[g, n:] = q_idx[g, n - 1] if n > 0 else 7
                else:
                    q_idx[g, n:] = rng.integers(0, 50, size=tok_cap - n)
            out.append((pattern, n_tok, q_idx))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# mhr_nce_log_counters
# ----------------------------------------------------------------------------------------------------------------------
COUNTER_G = 3
COUNTER_TOK_CAPS = [32, 1024, 1056, (140000 + 31) // 32 * 32]     # the last: more than 128 workgroups x 256 threads
COUNTER_GROUPS = [0, 2]
COUNTER_KS = [1, 5, 10, 50, 200]
COUNTER_N_K = [0, 1, 5]
COUNTER_FILLS = ["none", "part", "full"]


def counter_tables(tok_cap, fill):
    """(n_valid, rank, o_idx [G, tok_cap] int32, n_tok [G]).  Groups 0 and 2 mix the offsets 0 .. 3; group 1 holds no offset-0 token.
    Behind n_tok every entry is (n_valid 7, rank 0, offset 0): counted, if the bound were wrong."""
    rng = np.random.default_rng(tok_cap + len(fill))
    G = COUNTER_G
    n = {"none": [0] * G, "part": [tok_cap // 2 + 1, tok_cap // 3, tok_cap - 1], "full": [tok_cap] * G}[fill]
    n_tok = np.array(n, dtype=np.int32)
    n_valid = rng.integers(0, 1001, size=(G, tok_cap)).astype(np.int32)
    rank = rng.integers(0, 300, size=(G, tok_cap)).astype(np.int32)
    o_idx = rng.integers(0, 4, size=(G, tok_cap)).astype(np.int32)
    o_idx[1] = rng.integers(1, 4, size=tok_cap)
    for g in range(G):
        n_valid[g, n_tok[g]:], rank[g, n_tok[g]:], o_idx[g, n_tok[g]:] = 7, 0, 0
    return n_valid, rank, o_idx, n_tok


def counter_tables_u64():
    """One group of 4096 offset-0 tokens with n_valid just below 2^31: the sum needs more than 32 bits."""
    rng = np.random.default_rng(9)
    cap = 4096
    n_valid = ((1 << 31) - 1 - rng.integers(0, 1000, size=(1, cap))).astype(np.int32)
    rank = rng.integers(0, 300, size=(1, cap)).astype(np.int32)
    return n_valid, rank, np.zeros((1, cap), dtype=np.int32), np.array([cap], dtype=np.int32)
