"""The numpy oracles of tests/index_maps_data.py against a second, independent formulation each (torch.nonzero and boolean
indexing, torch.unique_consecutive, a plain Python loop), on every case list tests/test_gpu_index_maps.py runs - so that the GPU
comparisons do not rest on one reading of include/mhr.h - and the conditions the cases are meant to meet: the row capacity's
precondition, truncating token capacities, overflowing row capacities, a counter sum past 32 bits.  CPU only, all exact."""
import numpy as np
import pytest
import torch

import index_maps_data as D


def _eq(a, b):
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b))


# ----------------------------------------------------------------------------------------------------------------------
# packing maps
# ----------------------------------------------------------------------------------------------------------------------
def _pack_second(valid, cap):
    v = torch.from_numpy(valid != 0)
    B, L = v.shape
    nz = torch.nonzero(v)                                   # [total, 2] = (b, l) in window order
    total = nz.shape[0]
    kept = nz[:cap]
    src_of = torch.full((cap,), -1, dtype=torch.int64)
    src_of[:kept.shape[0]] = kept[:, 0] * L + kept[:, 1]
    cu = torch.zeros(B + 1, dtype=torch.int64)
    cu[1:] = torch.bincount(kept[:, 0], minlength=B).cumsum(0)
    number = torch.arange(total)
    row_of = torch.full((B, L), -1, dtype=torch.int64)
    row_of[v] = torch.where(number < cap, number, torch.full_like(number, -1))
    return cu.numpy(), src_of.numpy(), row_of.view(-1).numpy(), total if total > cap else 0


@pytest.mark.parametrize("B,L", D.PACK_SHAPES)
def test_pack_maps_oracle_and_its_capacities(B, L):
    for kind in D.PACK_MASKS:
        valid = D.pack_mask(B, L, kind)
        total = int((valid != 0).sum())
        assert valid.dtype == np.uint8 and valid.shape == (B, L)
        if kind == "bytes":
            assert set(np.unique(valid)) <= {0, *D.LIVE_BYTES}
        if kind == "mixed" and B >= 2:
            assert valid[0].sum() == 0 and valid[1].all()
        caps = D.pack_caps(valid)
        names = [n for n, _, _ in caps]
        assert len(set(c for _, c, _ in caps)) == len(caps) and all(c >= 1 for _, c, _ in caps)
        if total > 0:
            assert {"exact", "slack1", "slack3000"} <= set(names)
        for name, cap, over in caps:
            assert (total > cap) == over, (kind, name, total, cap)          # an overflow case really overflows
            cu, src_of, row_of, overflow = D.pack_maps_oracle(valid, cap)
            cu2, src2, row2, ov2 = _pack_second(valid, cap)
            _eq(cu, cu2), _eq(src_of, src2), _eq(row_of, row2)
            assert overflow == ov2 == (total if over else 0)
            assert cu.dtype == src_of.dtype == row_of.dtype == np.int32
            if name == "mid":                                                # the cut falls inside a sequence ...
                assert cap not in np.cumsum((valid != 0).sum(1)).tolist()
            if name == "edge":                                               # ... or exactly between two
                assert cap in np.cumsum((valid != 0).sum(1)).tolist()


def test_pack_case_lists_cover_the_cuts():
    """Every overflowing kind of capacity occurs; the slack of 3000 rows is more than one pass of the tail clear."""
    seen = set()
    for B, L in D.PACK_SHAPES:
        for kind in D.PACK_MASKS:
            seen |= {n for n, _, _ in D.pack_caps(D.pack_mask(B, L, kind))}
    assert seen == {"exact", "slack1", "slack3000", "short1", "mid", "edge", "one"}
    assert 3000 > 16 * 64


def test_guard_oracle():
    g = [0, 0, 0, 0]
    for total, cap, want in ((10, 10, [0, 0, 0, 0]), (10, 9, [1, 10, 9, 0]), (10, 4, [2, 10, 9, 0]), (12, 11, [3, 12, 11, 0]),
                             (5, 50, [3, 12, 11, 0])):
        g = D.guard_oracle(g, total, cap)
        assert g == want


# ----------------------------------------------------------------------------------------------------------------------
# masked row gather
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out", D.GATHER_N_OUT + [D.GATHER_N_OUT_LONG])
def test_gather_oracle_and_index_patterns(n_out):
    src = np.random.default_rng(n_out).integers(-2 ** 31, 2 ** 31, size=(D.GATHER_N_SRC, 8)).astype(np.int32)
    for pattern in D.GATHER_PATTERNS:
        idx = D.gather_idx(n_out, D.GATHER_N_SRC, pattern)
        assert idx.dtype == np.int32 and idx.shape == (n_out,) and idx.min() >= -1 and idx.max() < D.GATHER_N_SRC
        if pattern == "none":
            assert (idx == -1).all()
        if pattern in ("all", "dup"):
            assert (idx >= 0).all()
        if pattern == "mixed" and n_out > 1:
            assert (idx == -1).any()
        if pattern == "dup" and n_out > 3:
            assert len(set(idx.tolist())) < n_out
        t_idx, t_src = torch.from_numpy(idx).long(), torch.from_numpy(src)
        want = torch.where((t_idx >= 0)[:, None], t_src[t_idx.clamp(min=0)], torch.zeros((), dtype=torch.int32))
        _eq(D.gather_masked_oracle(src, idx), want.numpy())
    assert D.GATHER_N_OUT_LONG > 8192 * 16


# ----------------------------------------------------------------------------------------------------------------------
# token compaction
# ----------------------------------------------------------------------------------------------------------------------
def _compact_second(mask, q_all, p_all, o_all, tok_cap):
    m = torch.from_numpy(mask != 0)
    out = []
    for g in range(m.shape[0]):
        pos = torch.cumsum(m[g].long(), 0) - 1
        tos = torch.where(m[g] & (pos < tok_cap), pos, torch.full_like(pos, -1))
        out.append((torch.nonzero(m[g]).flatten()[:tok_cap].numpy(), torch.from_numpy(q_all)[g][m[g]][:tok_cap].numpy(),
                    torch.from_numpy(p_all)[m[g]][:tok_cap].numpy(), torch.from_numpy(o_all)[m[g]][:tok_cap].numpy(),
                    min(int(m[g].sum()), tok_cap), tos.numpy()))
    return out


def _check_compact(mask, tables, tok_cap):
    res = D.compact_oracle(mask, *tables, tok_cap)
    for g, (slots, q, p, o, n, tos) in enumerate(_compact_second(mask, *tables, tok_cap)):
        _eq(res["slots"][g], slots), _eq(res["q"][g], q), _eq(res["p"][g], p), _eq(res["o"][g], o)
        assert int(res["n_tok"][g]) == n == len(res["slots"][g])
        _eq(res["tok_of_slot"][g], tos)
    assert res["bad"] == 0
    return res


@pytest.mark.parametrize("G,n_slots", D.COMPACT_SHAPES)
def test_compact_oracle_default_capacity(G, n_slots):
    tables = D.compact_tables(G, n_slots)
    assert tables[0].shape == (G, n_slots) and all(t.dtype == np.int32 for t in tables)
    for kind in D.COMPACT_MASKS:
        mask = D.compact_mask(G, n_slots, kind)
        assert mask.dtype == np.uint8 and mask.shape == (G, n_slots)
        live = {"dead": 0, "live": n_slots}.get(kind)
        if live is not None:
            assert (mask != 0).sum() == G * live
        if kind == "edges" and n_slots > D.CHUNK:
            assert np.flatnonzero(mask[0])[:2].tolist() == [D.CHUNK - 1, D.CHUNK]
        _check_compact(mask, tables, (n_slots + 31) // 32 * 32)


def test_compact_shapes_reach_both_count_paths_and_the_chunk_stride():
    assert (2, 4136) in D.COMPACT_SHAPES and 4136 % 16 != 0 and 4136 // 16 * 16 > D.CHUNK     # group 1 misaligned, full threads exist
    assert max(n for _, n in D.COMPACT_SHAPES) > 64 * D.CHUNK


@pytest.mark.parametrize("G,n_slots,kind,tok_cap", D.COMPACT_CUT)
def test_compact_oracle_truncating_capacity(G, n_slots, kind, tok_cap):
    mask = D.compact_mask(G, n_slots, kind)
    assert ((mask != 0).sum(axis=1) > tok_cap).all()                        # a truncation case really truncates
    res = _check_compact(mask, D.compact_tables(G, n_slots), tok_cap)
    assert (res["n_tok"] == tok_cap).all() and res["tok_of_slot"].max() == tok_cap - 1
    for g in range(G):
        assert (res["tok_of_slot"][g, np.flatnonzero(mask[g])[tok_cap:]] == -1).all()


@pytest.mark.parametrize("G,n_slots", D.COMPACT_BYTES_SHAPES)
def test_compact_oracle_any_nonzero_byte_is_live(G, n_slots):
    mask = D.compact_mask(G, n_slots, "bytes")
    assert set(np.unique(mask)) == {0, *D.LIVE_BYTES}
    _check_compact(mask, D.compact_tables(G, n_slots), (n_slots + 31) // 32 * 32)
    same = D.compact_oracle((mask != 0).astype(np.uint8), *D.compact_tables(G, n_slots), n_slots)
    _eq(same["tok_of_slot"], D.compact_oracle(mask, *D.compact_tables(G, n_slots), n_slots)["tok_of_slot"])


@pytest.mark.parametrize("tok_cap", D.PACKED_TOK_CAPS)
def test_compact_oracle_packed_rows(tok_cap):
    valid, capacity, mask, q_all, p_all, o_all = D.packed_case()
    B, L, H, G = D.PACKED_B, D.PACKED_L, D.PACKED_H, D.PACKED_G
    n_slots = B * H * L
    assert 0 < capacity < int(valid.sum())                                  # the row map drops rows
    row_of = D.pack_maps_oracle(valid, capacity)[2]
    stride = capacity + D.PACKED_STRIDE_PAD
    cap = (n_slots if tok_cap is None else tok_cap) + 31 & ~31
    res = D.compact_oracle(mask, q_all, p_all, o_all, cap, packed=(row_of, L, H, stride))
    plain = D.compact_oracle(mask, q_all, p_all, o_all, cap)
    bad = 0
    for g in range(G):
        _eq(res["slots"][g], plain["slots"][g]), _eq(res["p"][g], plain["p"][g]), _eq(res["o"][g], plain["o"][g])
        for j, w in enumerate(plain["q"][g].tolist()):                     # the window form (b H + h) L + l, slot by slot
            b, h, l = w // (H * L), w // L % H, w % L
            r = int(row_of[b * L + l])
            if r < 0 or r >= stride:
                bad, r = bad + 1, 0
            assert int(res["q"][g][j]) == h * stride + r
    assert res["bad"] == bad > 0
    if tok_cap is not None:                                                 # only the listed slots are counted
        assert (np.asarray(mask != 0).sum(axis=1) > cap).all()
        assert bad < D.compact_oracle(mask, q_all, p_all, o_all, n_slots, packed=(row_of, L, H, stride))["bad"]
    lost_valid = sum(int(valid.reshape(-1)[b * L + l] != 0 and row_of[b * L + l] < 0) for b in range(B) for l in range(L))
    assert lost_valid == D.PACKED_DROP                                      # some tokens lose their row to the capacity


# ----------------------------------------------------------------------------------------------------------------------
# row maps
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tok_cap", D.ROW_TOK_CAPS)
def test_row_maps_oracle_and_the_row_capacity(tok_cap):
    cases = D.row_cases(tok_cap)
    row_cap = D.row_cap_of(tok_cap)
    seen = set()
    for pattern, n_tok, q_idx in cases:
        assert q_idx.shape == (D.ROW_G, tok_cap) and q_idx.dtype == np.int32 and n_tok.shape == (D.ROW_G,)
        for g in range(D.ROW_G):
            n = int(n_tok[g])
            assert 0 <= n <= tok_cap
            seen.add((pattern, n))
            row_q, row_first, tok2row, n_row = D.row_maps_oracle(q_idx[g, :n])
            assert n_row + 1 <= row_cap                                     # the precondition of include/mhr.h
            assert row_first.shape == (n_row + 1,) and int(row_first[n_row]) == n and tok2row.shape == (n,)
            if n:
                vals, inv, counts = torch.unique_consecutive(torch.from_numpy(q_idx[g, :n]), return_inverse=True, return_counts=True)
                _eq(row_q, vals.numpy()), _eq(tok2row, inv.numpy()), _eq(row_first[:n_row], (counts.cumsum(0) - counts).numpy())
                assert n_row == vals.numel()
            else:
                assert n_row == 0 and row_first.tolist() == [0]
            heads = set(row_first[:n_row].tolist())
            if pattern == "own":
                assert n_row == n
            if pattern == "single":
                assert n_row == min(n, 1)
            if pattern == "runs" and n > 64:
                assert 1 < n / n_row < 8
            if pattern == "straddle":
                assert not any(c in heads for c in range(D.CHUNK, n, D.CHUNK))
            if pattern == "starts":
                assert all(c in heads for c in range(0, n, D.CHUNK))
                assert n <= 64 or sum(1 for h in heads if h % 16 == 0 and h % D.CHUNK) > 0
            if pattern == "aaba" and n_row > 2:
                assert len(set(row_q.tolist())) == 2 and (row_q[1:] != row_q[:-1]).all()
            if g % 2 == 0 and 0 < n < tok_cap:
                assert (q_idx[g, n:] == q_idx[g, n - 1]).all()             # the tail continues the last run ...
            if g % 2 == 1 and n + 64 < tok_cap:
                assert len(set(q_idx[g, n:].tolist())) > 2                  # ... or holds rows of its own
    wanted = [n for n in D.ROW_N_TOK if n <= tok_cap] + [tok_cap]
    assert seen >= {(p, n) for p in D.ROW_PATTERNS for n in wanted}


# ----------------------------------------------------------------------------------------------------------------------
# log counters
# ----------------------------------------------------------------------------------------------------------------------
def _counters_loop(n_valid, rank, o_idx, n_tok, group, ks):
    cnt, total, hits = 0, 0, [0] * len(ks)
    for t in range(int(n_tok[group])):
        if o_idx[group][t] != 0:
            continue
        cnt += 1
        total += int(n_valid[group][t])
        for i, k in enumerate(ks):
            hits[i] += 1 if rank[group][t] < k else 0
    return cnt, total, hits


@pytest.mark.parametrize("tok_cap", D.COUNTER_TOK_CAPS)
def test_log_counters_oracle(tok_cap):
    assert tok_cap % 32 == 0
    for fill in D.COUNTER_FILLS:
        n_valid, rank, o_idx, n_tok = D.counter_tables(tok_cap, fill)
        lists = [a.tolist() for a in (n_valid, rank, o_idx)]                # (plain lists: the loop below reads them item by item)
        for g in range(D.COUNTER_G):                                        # what sits behind n_tok would be counted
            n = int(n_tok[g])
            assert (o_idx[g, n:] == 0).all() and (rank[g, n:] == 0).all() and (n_valid[g, n:] == 7).all()
        assert {"none": (n_tok == 0).all(), "part": ((n_tok > 0) & (n_tok < tok_cap)).all(), "full": (n_tok == tok_cap).all()}[fill]
        for group in D.COUNTER_GROUPS + [1]:
            cnt, total, hits = _counters_loop(*lists, n_tok, group, D.COUNTER_KS)
            if group == 1:
                assert cnt == 0                                             # the group without an offset-0 token
            elif fill != "none":
                assert cnt > 0
            for n_k in D.COUNTER_N_K:
                got = D.log_counters_oracle(n_valid, rank, o_idx, n_tok, group, D.COUNTER_KS[:n_k])
                want = [total / max(cnt, 1)] + [h / max(cnt, 1) for h in hits[:n_k]]
                assert got.dtype == np.float32 and got.shape == (1 + n_k,)
                _eq(got, np.array(want, dtype=np.float64).astype(np.float32))
                if cnt == 0:
                    assert (got == 0.0).all()
    assert D.COUNTER_TOK_CAPS[-1] > 128 * 256


def test_log_counters_u64_case_sums_past_32_bits():
    n_valid, rank, o_idx, n_tok = D.counter_tables_u64()
    cnt, total, hits = _counters_loop(n_valid.tolist(), rank.tolist(), o_idx.tolist(), n_tok, 0, D.COUNTER_KS)
    assert total > 2 ** 32 and cnt == int(n_tok[0]) and int(n_valid.min()) > 2 ** 30
    got = D.log_counters_oracle(n_valid, rank, o_idx, n_tok, 0, D.COUNTER_KS)
    _eq(got, np.array([total / cnt] + [h / cnt for h in hits], dtype=np.float64).astype(np.float32))
    assert float(got[0]) > 2.0 ** 30                                        # (a sum cut to 32 bits would give a mean below 2^20)
