"""The integer index-map kernels against the numpy oracles of tests/index_maps_data.py, bit for bit (no tolerance anywhere):

  * mhr_seq_pack_maps / mhr_seq_pack_maps_guarded (csrc/rows_pack.hip): all four outputs in full over shapes on both sides of one
    sequence per scan thread, empty / full / byte-valued masks, and capacities that fit, leave a long tail to clear, or cut the
    batch inside a sequence, between two, one row short and at 1; the guard words by the header's rule;
  * mhr_rows_gather_masked: f32 and bf16, dims below and beyond one pass of a wave's lanes, row counts around the 4 rows in flight
    and beyond one pass of the grid, written zeros proven against a NaN fill, both documented requirement failures;
  * mhr_token_compact (csrc/tokens.hip): sizes around the 16-slot thread and the 4096-slot chunk, a misaligned group, more than 64
    chunks, token capacities below the live count, mask bytes other than 0 / 1, packed head rows with lost rows counted;
  * mhr_row_maps: runs across and starting at chunk and thread boundaries, live counts around them, tails that must not show;
  * mhr_nce_log_counters: the stride loop, empty groups, a sum past 32 bits, back-to-back launches, the scratch left zero.
Where the header says "untouched" the C entry point is called with outputs pre-filled with a sentinel."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import index_maps_data as D

pytestmark = pytest.mark.gpu
CODE = os.path.join(ROOT, "multi-head-recommendation-with-human-priors_amd", "code")
SENT = D.SENTINEL


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if CODE not in sys.path:
        sys.path.insert(0, CODE)
    import mhr_amd  # noqa: F401
    from mhr_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def eq(got, want):
    np.testing.assert_array_equal(host(got) if torch.is_tensor(got) else np.asarray(got), np.asarray(want))


def filled(*shape):
    return torch.full(shape, SENT, dtype=torch.int32, device="cuda")


# ----------------------------------------------------------------------------------------------------------------------
# mhr_seq_pack_maps, mhr_seq_pack_maps_guarded
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", D.PACK_MASKS)
@pytest.mark.parametrize("B,L", D.PACK_SHAPES)
def test_seq_pack_maps_all_outputs(ops, B, L, kind):
    valid = D.pack_mask(B, L, kind)
    total = int((valid != 0).sum())
    kv = dev(valid)
    guard = torch.zeros(4, dtype=torch.int32, device="cuda")
    want_guard = [0, 0, 0, 0]
    for name, cap, over in D.pack_caps(valid):
        want = D.pack_maps_oracle(valid, cap)
        for g in (None, guard):
            cu, src_of, row_of, overflow = ops.seq_pack_maps(kv, B, L, cap, guard=g)
            eq(cu, want[0]), eq(src_of, want[1]), eq(row_of, want[2])
            assert int(overflow) == want[3] == (total if over else 0), (name, cap)
        want_guard = D.guard_oracle(want_guard, total, cap)
        assert guard.tolist() == want_guard, (name, cap)
    ops.seq_pack_maps(kv, B, L, total + 1, guard=guard)                    # a fitting call clears nothing
    assert guard.tolist() == want_guard


# ----------------------------------------------------------------------------------------------------------------------
# mhr_rows_gather_masked
# ----------------------------------------------------------------------------------------------------------------------
DTYPES = {"f32": (torch.float32, torch.int32), "bf16": (torch.bfloat16, torch.int16)}


def _gather_rows(dtype_name, n_rows, dim, seed):
    """Random rows as a device tensor and as their bit patterns (numpy has no bf16: the oracle moves bits)."""
    dtype, bits = DTYPES[dtype_name]
    src = torch.randn(n_rows, dim, generator=torch.Generator().manual_seed(seed)).to(dtype)
    return src.cuda(), src.view(bits).numpy()


def _check_gather(ops, dtype_name, src, src_bits, n_out, pattern):
    dtype, bits = DTYPES[dtype_name]
    idx = D.gather_idx(n_out, src.shape[0], pattern)
    out = torch.full((n_out, src.shape[1]), float("nan"), dtype=dtype, device="cuda")
    got = ops.rows_gather_masked(src, dev(idx), out=out)
    assert got is out
    eq(out.view(bits), D.gather_masked_oracle(src_bits, idx))             # bit patterns: a row still NaN cannot pass
    return idx


@pytest.mark.parametrize("dtype_name,dim", [(n, d) for n in ("f32", "bf16") for d in D.GATHER_DIMS[n]])
def test_rows_gather_masked_dims_and_tails(ops, dtype_name, dim):
    src, src_bits = _gather_rows(dtype_name, D.GATHER_N_SRC, dim, dim)
    for n_out in D.GATHER_N_OUT:
        for pattern in D.GATHER_PATTERNS:
            _check_gather(ops, dtype_name, src, src_bits, n_out, pattern)
    idx = D.gather_idx(5, D.GATHER_N_SRC, "mixed")                         # the allocating form of the wrapper
    got = ops.rows_gather_masked(src, dev(idx))
    assert got.shape == (5, dim) and got.dtype == src.dtype
    eq(got.view(DTYPES[dtype_name][1]), D.gather_masked_oracle(src_bits, idx))


@pytest.mark.parametrize("dtype_name", ["f32", "bf16"])
def test_rows_gather_masked_beyond_one_grid_pass(ops, dtype_name):
    dim = D.GATHER_DIMS[dtype_name][0]
    src, src_bits = _gather_rows(dtype_name, D.GATHER_N_SRC, dim, 5)
    for pattern in D.GATHER_PATTERNS:
        _check_gather(ops, dtype_name, src, src_bits, D.GATHER_N_OUT_LONG, pattern)


@pytest.mark.parametrize("dtype_name,bad_dim,off", [("f32", 6, 1), ("bf16", 12, 2)])
def test_rows_gather_masked_requirements_raise(ops, dtype_name, bad_dim, off):
    dtype, _ = DTYPES[dtype_name]
    idx = dev(np.array([0, -1, 2], dtype=np.int32))
    with pytest.raises(RuntimeError, match="16-byte"):                     # a row that does not fill whole 16-byte pieces
        ops.rows_gather_masked(torch.zeros(4, bad_dim, dtype=dtype, device="cuda"), idx)
    dim = 16
    aligned = torch.zeros(4, dim, dtype=dtype, device="cuda")
    shifted = torch.zeros(4 * dim + 8, dtype=dtype, device="cuda")[off:off + 4 * dim].view(4, dim)     # 4 bytes off
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4 and aligned.data_ptr() % 16 == 0
    with pytest.raises(RuntimeError, match="aligned"):
        ops.rows_gather_masked(shifted, idx)
    shifted_out = torch.zeros(3 * dim + 8, dtype=dtype, device="cuda")[off:off + 3 * dim].view(3, dim)
    with pytest.raises(RuntimeError, match="aligned"):
        ops.rows_gather_masked(aligned, idx, out=shifted_out)
    assert float(shifted_out.float().abs().max()) == 0.0                   # refused before any launch


# ----------------------------------------------------------------------------------------------------------------------
# mhr_token_compact
# ----------------------------------------------------------------------------------------------------------------------
def _check_lists(got, want, G, sentinel_tail=False):
    q_idx, p_idx, o_idx, n_tok, tos = got
    eq(n_tok, want["n_tok"])
    eq(tos, want["tok_of_slot"])
    for g in range(G):
        n = int(want["n_tok"][g])
        eq(q_idx[g, :n], want["q"][g]), eq(p_idx[g, :n], want["p"][g]), eq(o_idx[g, :n], want["o"][g])
        if sentinel_tail:                                                   # "entries >= n_tok[g] are left untouched"
            for t in (q_idx, p_idx, o_idx):
                assert bool((t[g, n:] == SENT).all())


@pytest.mark.parametrize("kind", D.COMPACT_MASKS)
@pytest.mark.parametrize("G,n_slots", D.COMPACT_SHAPES)
def test_token_compact_default_capacity(ops, G, n_slots, kind):
    mask = D.compact_mask(G, n_slots, kind)
    tables = D.compact_tables(G, n_slots)
    m = dev(mask)
    got = ops.token_compact(m if kind != "sparse" else m.view(torch.bool), *(dev(t) for t in tables), slot_map=True)
    cap = (n_slots + 31) // 32 * 32
    assert got[0].shape == (G, cap)
    _check_lists(got, D.compact_oracle(mask, *tables, cap), G)


def _compact_raw(ops, mask, tables, tok_cap):
    """The C entry point with sentinel-filled outputs."""
    G, n_slots = mask.shape
    m, q_all, p_all, o_all = dev(mask), dev(tables[0]), dev(tables[1]), dev(tables[2])
    q_idx, p_idx, o_idx = filled(G, tok_cap), filled(G, tok_cap), filled(G, tok_cap)
    n_tok, tos = filled(G), filled(G, n_slots)
    scratch = torch.empty(G, (n_slots + D.CHUNK - 1) // D.CHUNK, dtype=torch.int32, device="cuda")
    ops.lib.call("mhr_token_compact", m.data_ptr(), q_all.data_ptr(), p_all.data_ptr(), o_all.data_ptr(), G, n_slots, tok_cap,
                 q_idx.data_ptr(), p_idx.data_ptr(), o_idx.data_ptr(), n_tok.data_ptr(), scratch.data_ptr(), tos.data_ptr(),
                 0, 0, 0, 0, torch.cuda.current_stream().cuda_stream)
    return q_idx, p_idx, o_idx, n_tok, tos


@pytest.mark.parametrize("G,n_slots,kind,tok_cap", D.COMPACT_CUT)
def test_token_compact_capacity_below_the_live_count(ops, G, n_slots, kind, tok_cap):
    mask = D.compact_mask(G, n_slots, kind)
    tables = D.compact_tables(G, n_slots)
    want = D.compact_oracle(mask, *tables, tok_cap)
    assert (want["n_tok"] == tok_cap).all()
    _check_lists(ops.token_compact(dev(mask), *(dev(t) for t in tables), tok_cap=tok_cap, slot_map=True), want, G)
    _check_lists(_compact_raw(ops, mask, tables, tok_cap), want, G, sentinel_tail=True)


@pytest.mark.parametrize("G,n_slots", D.COMPACT_SHAPES)
def test_token_compact_leaves_the_tail_untouched(ops, G, n_slots):
    mask = D.compact_mask(G, n_slots, "sparse")
    tables = D.compact_tables(G, n_slots)
    cap = (n_slots + 31) // 32 * 32
    _check_lists(_compact_raw(ops, mask, tables, cap), D.compact_oracle(mask, *tables, cap), G, sentinel_tail=True)


@pytest.mark.parametrize("G,n_slots", D.COMPACT_BYTES_SHAPES)
def test_token_compact_any_nonzero_byte_is_live(ops, G, n_slots):
    """Mask bytes drawn from {1, 2, 0x80, 0xFF}: the chunk counts (16 bytes at a time where the group is aligned, byte by byte
    where it is not) must agree with the scatter, which takes any nonzero byte as live."""
    mask = D.compact_mask(G, n_slots, "bytes")
    tables = D.compact_tables(G, n_slots)
    cap = (n_slots + 31) // 32 * 32
    want = D.compact_oracle(mask, *tables, cap)
    _check_lists(ops.token_compact(dev(mask), *(dev(t) for t in tables), slot_map=True), want, G)
    _check_lists(_compact_raw(ops, mask, tables, cap), want, G, sentinel_tail=True)


@pytest.mark.parametrize("tok_cap", D.PACKED_TOK_CAPS)
def test_token_compact_packed_rows_and_lost_rows(ops, tok_cap):
    valid, capacity, mask, q_all, p_all, o_all = D.packed_case()
    B, L, H, G = D.PACKED_B, D.PACKED_L, D.PACKED_H, D.PACKED_G
    cu, src_of, row_of, overflow = ops.seq_pack_maps(dev(valid), B, L, capacity)
    want_row_of = D.pack_maps_oracle(valid, capacity)[2]
    eq(row_of, want_row_of)
    assert int(overflow) == int(valid.sum())
    stride = capacity + D.PACKED_STRIDE_PAD
    cap = ((B * H * L if tok_cap is None else tok_cap) + 31) // 32 * 32
    want = D.compact_oracle(mask, q_all, p_all, o_all, cap, packed=(want_row_of, L, H, stride))
    ops.bad_id_count()                                                      # read = clear
    got = ops.token_compact(dev(mask), dev(q_all), dev(p_all), dev(o_all), tok_cap=tok_cap, slot_map=True,
                            packed=(row_of, L, H, stride))
    _check_lists(got, want, G)
    assert ops.bad_id_count() == want["bad"] > 0
    assert ops.bad_id_count() == 0


# ----------------------------------------------------------------------------------------------------------------------
# mhr_row_maps
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tok_cap", D.ROW_TOK_CAPS)
def test_row_maps(ops, tok_cap):
    G, row_cap, pad = D.ROW_G, D.row_cap_of(tok_cap), 64
    scratch = torch.empty(G, (tok_cap + D.CHUNK - 1) // D.CHUNK, dtype=torch.int32, device="cuda")
    for pattern, n_tok, q_idx in D.row_cases(tok_cap):
        q, nt = dev(q_idx), dev(n_tok)
        row_q, row_first, n_row = filled(G, row_cap), filled(G, row_cap), filled(G)
        t2r_buf = filled(G * tok_cap + pad)                                 # (a strip behind tok2row that must stay as it is)
        ops.lib.call("mhr_row_maps", q.data_ptr(), nt.data_ptr(), G, tok_cap, row_cap, row_q.data_ptr(), row_first.data_ptr(),
                     t2r_buf.data_ptr(), n_row.data_ptr(), scratch.data_ptr(), torch.cuda.current_stream().cuda_stream)
        row_q, row_first, n_row, t2r_buf = host(row_q), host(row_first), host(n_row), host(t2r_buf)
        tok2row = t2r_buf[:G * tok_cap].reshape(G, tok_cap)
        assert (t2r_buf[G * tok_cap:] == SENT).all()
        for g in range(G):
            n, where = int(n_tok[g]), (pattern, tok_cap, n_tok.tolist(), g)
            w_q, w_first, w_t2r, w_n = D.row_maps_oracle(q_idx[g, :n])
            assert int(n_row[g]) == w_n, where
            np.testing.assert_array_equal(row_q[g, :w_n], w_q, err_msg=str(where))
            np.testing.assert_array_equal(row_first[g, :w_n + 1], w_first, err_msg=str(where))
            np.testing.assert_array_equal(tok2row[g, :n], w_t2r, err_msg=str(where))
            assert (tok2row[g, n:] == 0).all(), where                      # 0 beyond n_tok
            assert (row_q[g, w_n:] == SENT).all() and (row_first[g, w_n + 1:] == SENT).all(), where    # rows >= n_row untouched


# ----------------------------------------------------------------------------------------------------------------------
# mhr_nce_log_counters
# ----------------------------------------------------------------------------------------------------------------------
def _scratch_is_zero(ops):
    return len(ops._COUNTER_SCRATCH) > 0 and all(int(t.abs().max()) == 0 for t in ops._COUNTER_SCRATCH.values())


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("tok_cap", D.COUNTER_TOK_CAPS)
def test_nce_log_counters(ops, tok_cap):
    for fill in D.COUNTER_FILLS:
        tables = D.counter_tables(tok_cap, fill)
        n_valid, rank, o_idx, n_tok = (dev(t) for t in tables)
        for group in D.COUNTER_GROUPS + [1]:
            for n_k in D.COUNTER_N_K:
                ks = D.COUNTER_KS[:n_k]
                got = host(ops.nce_log_counters(n_valid, rank, o_idx, n_tok, group, ks))
                want = D.log_counters_oracle(*tables, group, ks)
                np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=str((fill, group, n_k, got, want)))
                if group == 1 or fill == "none":                            # no offset-0 token: every output is 0.0
                    assert (_bits(got) == 0).all()
                assert _scratch_is_zero(ops)


def test_nce_log_counters_sum_past_32_bits(ops):
    tables = D.counter_tables_u64()
    got = host(ops.nce_log_counters(*(dev(t) for t in tables), 0, D.COUNTER_KS))
    want = D.log_counters_oracle(*tables, 0, D.COUNTER_KS)
    assert float(want[0]) > 2.0 ** 30
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert _scratch_is_zero(ops)


def test_nce_log_counters_back_to_back(ops):
    """Three launches in a row, nothing read in between: each gives its own answer and the shared scratch ends zero."""
    tok_cap = D.COUNTER_TOK_CAPS[-1]
    tables = D.counter_tables(tok_cap, "part")
    n_valid, rank, o_idx, n_tok = (dev(t) for t in tables)
    calls = [(0, D.COUNTER_KS), (2, D.COUNTER_KS[:1]), (1, D.COUNTER_KS[:3])]
    torch.cuda.synchronize()
    outs = [ops.nce_log_counters(n_valid, rank, o_idx, n_tok, group, ks) for group, ks in calls]
    for out, (group, ks) in zip(outs, calls):
        np.testing.assert_array_equal(_bits(host(out)), _bits(D.log_counters_oracle(*tables, group, ks)))
    assert _scratch_is_zero(ops)
