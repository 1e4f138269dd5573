"""Thin torch-facing wrappers over the C ABI (include/mhr.h).

PyTorch is plumbing here: device memory (`Tensor.data_ptr()`), the current HIP stream and
`torch.distributed`.  Every function enqueues hand-written gfx950 kernels from libmhr_hip.so on the
current stream; none of them synchronises, and none has a CPU or eager fallback.
"""
import collections
import os
import types

import torch

from . import lib

F32, BF16 = lib.F32, lib.BF16

# Optional per-launch timing (bench.py): when PROFILE is a dict, calls named in it are bracketed by HIP events
# recorded on the stream the kernel is launched on; durations are read after a sync by `profile_summary`.
PROFILE = None


def _timed_call(name, *args, entry=None):
    """`entry`: the C entry point to call when it is not `name` (a stage that changed its kernel keeps its name in the profile)."""
    entry = entry or name
    if PROFILE is not None and name in PROFILE:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lib.call(entry, *args)
        e1.record()
        PROFILE[name].append((e0, e1))
    else:
        lib.call(entry, *args)


def profile_summary(with_max=False):
    """name -> (launches, mean ms, total ms[, max ms]); call after torch.cuda.synchronize()."""
    out = {}
    for name, evs in (PROFILE or {}).items():
        if evs:
            ms = [a.elapsed_time(b) for a, b in evs]
            out[name] = (len(ms), sum(ms) / len(ms), sum(ms)) + ((max(ms),) if with_max else ())
    return out


def profile_raw(name):
    """Every measured duration (ms) of one entry point, in launch order."""
    return [a.elapsed_time(b) for a, b in (PROFILE or {}).get(name, [])]


def _dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t.dtype} (float32 / bfloat16 only)")


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream():
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())




def zeros_many(dev, *specs):
    """Several zero-initialised 4-byte tensors from ONE allocation and ONE fill launch (each small `torch.zeros` is its own
    fill kernel: about 4.5 us of device timeline apiece, and a training step used to issue some forty of them).
    specs: (shape, dtype) with dtype float32 / int32; every tensor starts 16-byte aligned."""
    sizes = []
    for shape, dtype in specs:
        n = 1
        for d in shape:
            n *= int(d)
        sizes.append((n + 3) // 4 * 4)
    buf = torch.zeros(max(sum(sizes), 4), dtype=torch.int32, device=dev)
    out, off = [], 0
    for (shape, dtype), sz in zip(specs, sizes):
        n = 1
        for d in shape:
            n *= int(d)
        t = buf[off:off + n]
        out.append((t if dtype == torch.int32 else t.view(dtype)).view(*shape))
        off += sz
    return out


def _chk(t, name, dtype=None):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor; the MI355X path has no CPU fallback")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t


# ------------------------------------------------------------------------------------------------
# embedding
# ------------------------------------------------------------------------------------------------
def embedding_gather(table, ids, out_dtype=torch.bfloat16, pos_table=None, seq_len=0, x_dtype=torch.float32,
                     want_rows=True, out=None, window=None, n_x_ids=0):
    """rows = table[ids] (-> [*ids.shape, D]); with pos_table also x = table[ids[:, :seq_len]] + pos[:seq_len].
    `out`: optional preallocated contiguous [ids.numel(), D] destination (e.g. a slice of a larger row matrix)."""
    _chk(table, "table", torch.float32)
    _chk(ids, "ids", torch.int64)
    D = table.shape[1]
    n = ids.numel()
    if out is not None:
        _chk(out, "out")
        assert out.numel() == n * D
    elif want_rows:
        out = torch.empty(*ids.shape, D, dtype=out_dtype, device=table.device)
    x = None
    # `window` / `n_x_ids`: flat ids whose first n_x_ids entries are [n_x_ids / window, window] item windows (they get
    # the position-added x), followed by ids that only need their rows (the negative pools): one launch for both
    if window is None:
        window = ids.shape[-1] if pos_table is not None else 0
    if pos_table is not None:
        _chk(pos_table, "pos_table", torch.float32)
        if n_x_ids:
            x = torch.empty(n_x_ids // window, seq_len, D, dtype=x_dtype, device=table.device)
        else:
            x = torch.empty(*ids.shape[:-1], seq_len, D, dtype=x_dtype, device=table.device)
    _timed_call("mhr_embedding_gather_fwd", table.data_ptr(), table.shape[0], D, ids.data_ptr(), n,
             _ptr(out), _dt(out) if out is not None else F32, _ptr(pos_table), seq_len, window,
             _ptr(x), _dt(x) if x is not None else F32, int(n_x_ids), _stream())
    return out, x


def embedding_scatter_add(grad_rows, ids, grad_table):
    _chk(grad_rows, "grad_rows")
    _chk(ids, "ids", torch.int64)
    _chk(grad_table, "grad_table", torch.float32)
    lib.call("mhr_embedding_scatter_add_bwd", grad_rows.data_ptr(), _dt(grad_rows), ids.data_ptr(), ids.numel(),
             grad_table.data_ptr(), grad_table.shape[0], grad_table.shape[1], _stream())
    return grad_table


def sparse_rows_segment_sum(sorted_ids, perm, grad_a, grad_b, x_grad, seq_len, window_len, out_rows, row_slot, x_row_of=None):
    """x_row_of (int32 [B * seq_len], seq_pack_maps' row_of): x_grad is the PACKED [capacity, D] gradient of the encoder input."""
    D = out_rows.shape[-1]
    if x_row_of is not None:
        _chk(x_row_of, "x_row_of", torch.int32)
        assert x_grad is not None and grad_a is not None and x_row_of.numel() == grad_a.numel() // D // window_len * seq_len
    n_a = 0 if grad_a is None else grad_a.numel() // D
    n_b = 0 if grad_b is None else grad_b.numel() // D
    _timed_call("mhr_sparse_rows_segment_sum", sorted_ids.data_ptr(), perm.data_ptr(), sorted_ids.numel(),
             _ptr(grad_a), _dt(grad_a) if grad_a is not None else F32, n_a,
             _ptr(grad_b), _dt(grad_b) if grad_b is not None else F32, n_b,
             _ptr(x_grad), seq_len, window_len, _ptr(x_row_of), out_rows.data_ptr(), row_slot.data_ptr(), row_slot.numel(), D,
             _stream())


def pos_grad_packed(d_x, row_of, B, L, out):
    """out [>= L, D] fp32 += the position table's gradient from the PACKED encoder-input gradient d_x [capacity, D]:
    out[l] += sum_b d_x[row_of[b L + l]] (mhr_pos_grad_packed; fixed order, no atomics)."""
    _chk(d_x, "d_x", torch.float32)
    _chk(row_of, "row_of", torch.int32)
    _chk(out, "out", torch.float32)
    D = d_x.shape[-1]
    assert row_of.numel() == B * L and out.numel() >= L * D
    lib.call("mhr_pos_grad_packed", d_x.data_ptr(), row_of.data_ptr(), int(B), int(L), D, out.data_ptr(), _stream())
    return out


def window_rows_add_packed(rows, window, L, d_x, row_of, out=None):
    """The item windows' gradient rows [B * window, D] fp32 with the packed input-side gradient d_x [capacity, D] added at the
    valid positions (row_of [B * L]), written to `out` (default: a new tensor); `rows` is left as it came."""
    _chk(rows, "rows", torch.float32)
    _chk(d_x, "d_x", torch.float32)
    _chk(row_of, "row_of", torch.int32)
    D = rows.shape[-1]
    n = rows.numel() // D
    assert n % window == 0 and row_of.numel() == n // window * L
    if out is None:
        out = torch.empty_like(rows)
    _chk(out, "out", torch.float32)
    assert out.shape == rows.shape
    lib.call("mhr_window_rows_add_packed", rows.data_ptr(), n, int(window), int(L), d_x.data_ptr(), row_of.data_ptr(), D,
             out.data_ptr(), _stream())
    return out


def adam_rows(w, m, v, grad_rows, row_slot, step, lr, grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
              scale_dev=None):
    """scale_dev (device float[2], `grad_clip_coef`'s record): the gradient scale is scale_dev[1] instead of grad_scale."""
    if scale_dev is not None:
        _timed_call("mhr_adam_rows_scaled", w.data_ptr(), m.data_ptr(), v.data_ptr(), w.shape[0], w.shape[1],
                    grad_rows.data_ptr(), _ptr(row_slot), grad_scale, lr, betas[0], betas[1], eps, weight_decay, step,
                    _chk(scale_dev, "scale_dev", torch.float32).data_ptr(), _stream())
        return
    _timed_call("mhr_adam_rows", w.data_ptr(), m.data_ptr(), v.data_ptr(), w.shape[0], w.shape[1], grad_rows.data_ptr(),
             _ptr(row_slot), grad_scale, lr, betas[0], betas[1], eps, weight_decay, step, _stream())


def adam_flat(w, g, m, v, step, lr, grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, w_bf16=None,
              hist=None, step_dev=None, hist_len=64, scale_dev=None):
    """hist [hist_len, 4] f32 + step_dev int64[1] (device): the step's constants come from device memory (hipGraph replay).
    scale_dev (device float[2], `grad_clip_coef`'s record): the gradient scale is scale_dev[1] instead of grad_scale."""
    if scale_dev is not None:
        _timed_call("mhr_adam_flat_scaled", w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), w.numel(), grad_scale, lr,
                    betas[0], betas[1], eps, weight_decay, step, _ptr(w_bf16), _ptr(hist), 0 if hist is None else hist_len,
                    _ptr(step_dev), _chk(scale_dev, "scale_dev", torch.float32).data_ptr(), _stream())
        return
    lib.call("mhr_adam_flat", w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), w.numel(), grad_scale, lr,
             betas[0], betas[1], eps, weight_decay, step, _ptr(w_bf16), _ptr(hist), 0 if hist is None else hist_len,
             _ptr(step_dev), _stream())


ADAM_CHUNK = 8192         # elements of the flat buffer one workgroup of mhr_adam_flat_groups owns at a time (AG_CHUNK)
ADAM_MAX_GROUPS = 16


def adam_group_segments(sizes, groups, pad=8):
    """Host side of the static tables of `adam_flat_groups`, as plain lists: parameters of `sizes[i]` elements laid out back to
    back, each slot padded to `pad`, the whole buffer to 8; `groups[i]` the group of parameter i.  Consecutive parameters of one
    group merge into one segment (the closing padding belongs to the last one).  -> (seg_off [S + 1], seg_group [S],
    chunk_seg [ceil(n / 8192)]); an empty buffer has one empty segment of group 0."""
    assert len(sizes) == len(groups) and pad % 8 == 0
    seg_off, seg_group, off = [0], [], 0
    for sz, gr in zip(sizes, groups):
        if not seg_group or seg_group[-1] != int(gr):
            if seg_group:
                seg_off.append(off)
            seg_group.append(int(gr))
        off += (int(sz) + pad - 1) // pad * pad
    if not seg_group:
        seg_group.append(0)
    seg_off.append((off + 7) // 8 * 8)
    return seg_off, seg_group, adam_chunk_segments(seg_off)


def adam_chunk_segments(seg_off):
    """chunk_seg[c] = the segment that holds element c * 8192 (the last segment that starts at or before it and is not empty)."""
    n, out, s = seg_off[-1], [], 0
    for c in range((n + ADAM_CHUNK - 1) // ADAM_CHUNK):
        while seg_off[s + 1] <= c * ADAM_CHUNK:
            s += 1
        out.append(s)
    return out


AdamGroupTables = collections.namedtuple("AdamGroupTables", "seg_off seg_group chunk_seg n n_seg n_groups")


def adam_group_tables(seg_off, seg_group, n_groups, device):
    """The static tables of `adam_flat_groups` on the device, checked on the host first (the kernel trusts them): ascending
    offsets from 0 that are multiples of 8, groups in [0, n_groups), 1 <= n_groups <= 16."""
    seg_off, seg_group = [int(x) for x in seg_off], [int(x) for x in seg_group]
    if len(seg_group) < 1 or len(seg_off) != len(seg_group) + 1 or seg_off[0] != 0:
        raise ValueError("adam_group_tables: seg_off must hold len(seg_group) + 1 >= 2 offsets and start at 0")
    if any(o % 8 for o in seg_off) or any(b < a for a, b in zip(seg_off, seg_off[1:])):
        raise ValueError("adam_group_tables: seg_off must ascend in multiples of 8")
    if not 1 <= n_groups <= ADAM_MAX_GROUPS or any(not 0 <= x < n_groups for x in seg_group):
        raise ValueError(f"adam_group_tables: n_groups={n_groups} outside 1..{ADAM_MAX_GROUPS}, or a segment's group outside [0, n_groups)")
    chunk_seg = adam_chunk_segments(seg_off)
    return AdamGroupTables(torch.tensor(seg_off, dtype=torch.int64, device=device),
                           torch.tensor(seg_group, dtype=torch.int32, device=device),
                           torch.tensor(chunk_seg or [0], dtype=torch.int32, device=device),
                           seg_off[-1], len(seg_group), int(n_groups))


def adam_group_consts(out_row, step, lrs, weight_decays, betas=(0.9, 0.999), eps=1e-8):
    """out_row (HOST fp32 [n_groups, 4], contiguous) = one `mhr_adam_consts` row per group: the constants of step `step`."""
    assert not out_row.is_cuda and out_row.dtype == torch.float32 and out_row.is_contiguous()
    assert out_row.shape == (len(lrs), 4) and len(lrs) == len(weight_decays)
    for k, (lr, wd) in enumerate(zip(lrs, weight_decays)):
        lib.call("mhr_adam_consts", float(lr), betas[0], betas[1], eps, float(wd), int(step), out_row[k].data_ptr())
    return out_row


def adam_flat_groups(w, g, m, v, tables, gconst, step, grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8, w_bf16=None,
                     step_dev=None, scale_dev=None):
    """`adam_flat` with per-segment lr / weight decay in ONE launch (mhr_adam_flat_groups).  tables: `adam_group_tables`;
    gconst: device fp32 [hist_len, n_groups, 4], row step % hist_len filled by `adam_group_consts`; the kernel always reads its
    constants there - `step` (or step_dev[0], device int64, for a hipGraph-replayed step) only picks the row."""
    _chk(gconst, "gconst", torch.float32)
    if gconst.dim() != 3 or gconst.shape[1] != tables.n_groups or gconst.shape[2] != 4:
        raise ValueError(f"adam_flat_groups: gconst must be [hist_len, {tables.n_groups}, 4], got {tuple(gconst.shape)}")
    if w.numel() != tables.n or any(t.numel() != w.numel() for t in (g, m, v)) or (w_bf16 is not None and w_bf16.numel() != w.numel()):
        raise ValueError(f"adam_flat_groups: the tables cover {tables.n} elements, the buffers hold {w.numel()}")
    for t, name in ((w, "w"), (g, "g"), (m, "m"), (v, "v")):
        _chk(t, name, torch.float32)
    _timed_call("mhr_adam_flat_groups", w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), w.numel(), grad_scale,
                betas[0], betas[1], eps, int(step), _ptr(w_bf16), tables.seg_off.data_ptr(), tables.seg_group.data_ptr(),
                tables.n_seg, tables.chunk_seg.data_ptr(), gconst.data_ptr(), gconst.shape[0], tables.n_groups,
                _ptr(step_dev), _ptr(scale_dev), _stream())


def grad_sqnorm_partials(n, dim=1):
    """How many fp64 partials `grad_sqnorm_flat` over n elements (dim = 1) / `grad_sqnorm_rows` over n rows of `dim` writes
    (a host size query; 1 at n = 0)."""
    p = lib.load().mhr_grad_sqnorm_partials(int(n), int(dim))
    if p < 0:
        raise ValueError(f"grad_sqnorm_partials: bad sizes (n={n}, dim={dim})")
    return int(p)


def grad_sqnorm_flat(g, partials, off=0):
    """partials[off + k] (fp64) = the sum of squares of the k-th fixed range of the flat fp32 tensor g; returns the count."""
    _chk(g, "g", torch.float32)
    _chk(partials, "partials", torch.float64)
    n = g.numel()
    p = grad_sqnorm_partials(n)
    assert off >= 0 and off + p <= partials.numel(), "grad_sqnorm_flat: the partials buffer is too small"
    _timed_call("mhr_grad_sqnorm_flat", g.data_ptr(), n, partials.data_ptr(), int(off), _stream())
    return p


def grad_sqnorm_rows(rows, sorted_ids, n_rows, partials, off=0):
    """The same over the segment-head rows of a sparse row gradient (rows [n_ids, D] fp32, sorted_ids [n_ids] int64) whose id
    lies in [0, n_rows): the rows the table Adam applies.  Returns the count of partials written."""
    _chk(rows, "rows", torch.float32)
    _chk(sorted_ids, "sorted_ids", torch.int64)
    _chk(partials, "partials", torch.float64)
    n_ids, D = sorted_ids.numel(), rows.shape[-1]
    assert rows.numel() == n_ids * D
    p = grad_sqnorm_partials(n_ids, D)
    assert off >= 0 and off + p <= partials.numel(), "grad_sqnorm_rows: the partials buffer is too small"
    _timed_call("mhr_grad_sqnorm_rows", rows.data_ptr(), sorted_ids.data_ptr(), n_ids, D, int(n_rows), partials.data_ptr(),
                int(off), _stream())
    return p


def grad_clip_coef(partials, n_partials, pre_scale, max_norm, out2):
    """out2 (device float[2]) = {total_norm, pre_scale * min(1, max_norm / (total_norm + 1e-6))} with
    total_norm = sqrt(partials[:n_partials].sum()) * pre_scale - torch's clip_grad_norm_ coefficient, left on the device."""
    _chk(partials, "partials", torch.float64)
    _chk(out2, "out2", torch.float32)
    assert 0 <= n_partials <= partials.numel() and out2.numel() >= 2
    _timed_call("mhr_grad_clip_coef", partials.data_ptr(), int(n_partials), float(pre_scale), float(max_norm),
                out2.data_ptr(), _stream())
    return out2


def heads_residual_fwd(x, z, B, L, H):
    """out [B, H, L, D] f32 = x[b, l] + silu(z[b, l, h]);  x [B*L, D] f32, z [B*L, H*D] bf16."""
    _chk(x, "x", torch.float32)
    _chk(z, "z", torch.bfloat16)
    D = x.shape[-1]
    out = torch.empty(B, H, L, D, dtype=torch.float32, device=x.device)
    lib.call("mhr_heads_residual_fwd", x.data_ptr(), z.data_ptr(), out.data_ptr(), B * L, L, H, D, _stream())
    return out


def heads_residual_bwd(d_out, z, B, L, H):
    """(dz [B*L, H*D] bf16, dx [B*L, D] f32) from d_out [B, H, L, D] f32."""
    _chk(d_out, "d_out", torch.float32)
    D = d_out.shape[-1]
    dz = torch.empty_like(z)
    dx = torch.empty(B * L, D, dtype=torch.float32, device=z.device)
    lib.call("mhr_heads_residual_bwd", d_out.data_ptr(), z.data_ptr(), dz.data_ptr(), dx.data_ptr(), B * L, L, H, D, _stream())
    return dz, dx


def sum_rows_many(ptr_table, n, rows, cols, keep=None):
    """out_i += x_i.sum(0) for n equally shaped bf16 matrices in one launch; ptr_table: device int64 [2 n] (sources, then fp32
    destinations).  `keep`: the tensors behind the addresses (held by the caller until the launch is enqueued)."""
    _chk(ptr_table, "ptr_table", torch.int64)
    _timed_call("mhr_sum_rows_many", ptr_table.data_ptr(), int(n), int(rows), int(cols), _stream())


def bad_id_count(reset=True):
    """Ids outside the table that embedding gathers met since the last reset (they are clamped on the device, where the
    reference's nn.Embedding raises).  Synchronises: call it where the host reads device results anyway."""
    import ctypes
    c = ctypes.c_int64(0)
    lib.call("mhr_bad_id_count", ctypes.addressof(c), 1 if reset else 0)
    return int(c.value)


def sum_rows_into(x, out):
    """out [cols] fp32 += column sums of x [rows, cols] bf16 or fp32 (contiguous)."""
    _chk(out, "out", torch.float32)
    cols = out.numel()
    assert x.numel() % cols == 0
    if x.dtype == torch.float32:
        _chk(x, "x", torch.float32)
        lib.call("mhr_sum_rows_f32_into", x.data_ptr(), x.numel() // cols, cols, out.data_ptr(), _stream())
        return out
    _chk(x, "x", torch.bfloat16)
    _timed_call("mhr_sum_rows_into", x.data_ptr(), x.numel() // cols, cols, out.data_ptr(), _stream())
    return out


# ------------------------------------------------------------------------------------------------
# normalisation / gate
# ------------------------------------------------------------------------------------------------
def _out_like(out, shape, dtype, device, name):
    """`out` (a caller's buffer: same element count and dtype, contiguous) or a fresh tensor."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    n = 1
    for d in shape:
        n *= int(d)
    if out.dtype != dtype or out.numel() != n or not out.is_contiguous() or out.device != device:
        raise ValueError(f"{name}: expected a contiguous {dtype} buffer of {n} elements on {device}")
    return out


def layernorm_fwd(x, out_dtype=torch.bfloat16, eps=1e-6, out=None):
    _chk(x, "x")
    D = x.shape[-1]
    rows = x.numel() // D
    y = _out_like(out, x.shape, out_dtype, x.device, "layernorm_fwd out")
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    lib.call("mhr_layernorm_fwd", x.data_ptr(), _dt(x), y.data_ptr(), _dt(y), mean.data_ptr(), rstd.data_ptr(), rows, D,
             eps, _stream())
    return y, mean, rstd


def layernorm_bwd(dy, x, mean, rstd, dx=None, accumulate=False, dx_dtype=torch.float32):
    _chk(dy, "dy")
    D = x.shape[-1]
    rows = x.numel() // D
    if dx is None:
        dx = torch.empty(x.shape, dtype=dx_dtype, device=x.device)
    lib.call("mhr_layernorm_bwd", dy.data_ptr(), _dt(dy), x.data_ptr(), _dt(x), mean.data_ptr(), rstd.data_ptr(),
             dx.data_ptr(), _dt(dx), 1 if accumulate else 0, rows, D, _stream())
    return dx


def add_cast(x, y, out16=None):
    """(x + y fp32, its bf16 copy) for x fp32 and y bf16 of one shape, one pass (mhr_add_cast)."""
    _chk(x, "x", torch.float32)
    _chk(y, "y", torch.bfloat16)
    assert x.shape == y.shape
    out = torch.empty_like(x)
    out16 = _out_like(out16, y.shape, torch.bfloat16, y.device, "add_cast out16")
    lib.call("mhr_add_cast", x.data_ptr(), y.data_ptr(), out.data_ptr(), out16.data_ptr(), x.numel(), _stream())
    return out, out16


def _dead_args(dead, rows):
    """(first_row pointer, seq_len) of a `dead=(first_row [B] int32, L)` row-liveness descriptor (attn_seq_layout): rows in front
    of a sequence's first valid key are not loaded by the row-wise encoder kernels (they read as zeros, zeros are written)."""
    if dead is None:
        return 0, 0
    first_row, L = dead
    if first_row.dtype != torch.int32 or first_row.numel() * L != rows:
        raise ValueError("dead rows: first_row must be int32 [B] with B * L == rows")
    return first_row.data_ptr(), int(L)


def add_layernorm_fwd(x, y, eps=1e-6, xn_out=None, dead=None):
    """x_out = x + y (fp32 + bf16), xn = LN(x_out) bf16.  Returns (x_out, xn, mean, rstd)."""
    _chk(x, "x", torch.float32)
    _chk(y, "y", torch.bfloat16)
    D = x.shape[-1]
    rows = x.numel() // D
    x_out = torch.empty_like(x)
    xn = _out_like(xn_out, x.shape, torch.bfloat16, x.device, "add_layernorm_fwd xn_out")
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    lib.call("mhr_add_layernorm_fwd", x.data_ptr(), y.data_ptr(), x_out.data_ptr(), xn.data_ptr(), mean.data_ptr(),
             rstd.data_ptr(), rows, D, eps, *_dead_args(dead, rows), _stream())
    return x_out, xn, mean, rstd


def add_layernorm_bwd(d_xn, x_out, mean, rstd, d_xout, dy_out=None, dead=None):
    """-> (dx f32, dy bf16), both = d_xout + LN'(d_xn)."""
    _chk(d_xn, "d_xn", torch.bfloat16)
    _chk(d_xout, "d_xout", torch.float32)
    D = x_out.shape[-1]
    rows = x_out.numel() // D
    dx = torch.empty_like(x_out)
    dy = _out_like(dy_out, x_out.shape, torch.bfloat16, x_out.device, "add_layernorm_bwd dy_out")
    lib.call("mhr_add_layernorm_bwd", d_xn.data_ptr(), x_out.data_ptr(), mean.data_ptr(), rstd.data_ptr(), d_xout.data_ptr(),
             dx.data_ptr(), dy.data_ptr(), rows, D, *_dead_args(dead, rows), _stream())
    return dx, dy


def ln_gate_fwd(h, a, dim, out_dtype=None, eps=1e-6, dropout_p=0.0, seed=0, seed_dev=None, out=None, dead=None):
    """o = silu(h[:, :dim]) * LN(a) * dropmask.  h [rows, stride] pre-activation, a [rows, dim].
    seed_dev (device int64[1], optional): step counter of a hipGraph-replayed step; `seed` is then the per-layer part."""
    rows = a.numel() // dim
    o = _out_like(out, (rows, dim), out_dtype or a.dtype, a.device, "ln_gate_fwd out").view(rows, dim)
    mean = torch.empty(rows, dtype=torch.float32, device=a.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=a.device)
    assert h.dtype == a.dtype
    lib.call("mhr_ln_gate_fwd", h.data_ptr(), h.stride(0), a.data_ptr(), _dt(a), o.data_ptr(), _dt(o), mean.data_ptr(),
             rstd.data_ptr(), rows, dim, eps, dropout_p, seed, _ptr(seed_dev), *_dead_args(dead, rows), _stream())
    return o, mean, rstd


def ln_gate_bwd(d_o, h, a, mean, rstd, dh, dim, dropout_p=0.0, seed=0, seed_dev=None, dead=None):
    """writes du into dh[:, :dim]; returns da."""
    rows = a.numel() // dim
    da = torch.empty_like(a)
    lib.call("mhr_ln_gate_bwd", d_o.data_ptr(), _dt(d_o), h.data_ptr(), h.stride(0), a.data_ptr(), _dt(a), mean.data_ptr(),
             rstd.data_ptr(), dh.data_ptr(), dh.stride(0), da.data_ptr(), rows, dim, dropout_p, seed, _ptr(seed_dev),
             *_dead_args(dead, rows), _stream())
    return da


def l2norm_rows(x, out_dtype=torch.bfloat16, want_norms=False):
    _chk(x, "x")
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    norms = torch.empty(rows, dtype=torch.float32, device=x.device) if want_norms else None
    lib.call("mhr_l2norm_rows", x.data_ptr(), _dt(x), y.data_ptr(), _dt(y), _ptr(norms), rows, D, _stream())
    return (y, norms) if want_norms else y


def l2norm_rows_bwd(dy, x, norms):
    """dx of y = x / |x| (fp32 rows)."""
    _chk(dy, "dy", torch.float32)
    _chk(x, "x", torch.float32)
    D = x.shape[-1]
    dx = torch.empty_like(x)
    lib.call("mhr_l2norm_rows_bwd", dy.data_ptr(), x.data_ptr(), norms.data_ptr(), dx.data_ptr(), x.numel() // D, D, _stream())
    return dx


def embedding_gather_step(table, pos_table, ids_all, n_item_ids, seq_len, window, pack=None):
    """One launch for a training step's table reads: item windows -> (rows fp32 [n_item_ids, D], x fp32 [B, seq_len, D] with the
    position add); negative-pool ids -> (normalised bf16 rows [n_neg, D], norms fp32 [n_neg]).
    pack = (row_of, src_of, capacity) of seq_pack_maps: x is the PACKED encoder input [capacity, D] (valid positions back to back,
    zero rows behind them) - what rows_gather_masked would make of the window form, bit for bit, without the window form."""
    _chk(table, "table", torch.float32)
    _chk(pos_table, "pos_table", torch.float32)
    _chk(ids_all, "ids_all", torch.int64)
    D = table.shape[1]
    dev = table.device
    n = ids_all.numel()
    n_neg = n - n_item_ids
    rows = torch.empty(n_item_ids, D, dtype=torch.float32, device=dev)
    row_of = src_of = None
    cap = 0
    if pack is not None:
        row_of, src_of, cap = pack
        _chk(row_of, "row_of", torch.int32)
        _chk(src_of, "src_of", torch.int32)
        cap = int(cap)
        assert row_of.numel() == n_item_ids // window * seq_len and src_of.numel() == cap
        x = torch.empty(cap, D, dtype=torch.float32, device=dev)
    else:
        x = torch.empty(n_item_ids // window, seq_len, D, dtype=torch.float32, device=dev)
    negs = torch.empty(n_neg, D, dtype=torch.bfloat16, device=dev)
    norms = torch.empty(n_neg, dtype=torch.float32, device=dev)
    _timed_call("mhr_embedding_gather_step", table.data_ptr(), table.shape[0], D, ids_all.data_ptr(), n, n_item_ids, rows.data_ptr(),
                pos_table.data_ptr(), seq_len, window, x.data_ptr(), negs.data_ptr(), norms.data_ptr(), _ptr(row_of), _ptr(src_of),
                cap, _stream())
    return rows, x, negs, norms


def l2norm_rows_indexed_bwd(dy, table, ids, norms):
    """dx of y = table[ids] / |table[ids]| w.r.t. the gathered rows (fp32 [n, D]); the rows are re-read from the table."""
    _chk(dy, "dy", torch.float32)
    _chk(table, "table", torch.float32)
    _chk(ids, "ids", torch.int64)
    D = table.shape[1]
    dx = torch.empty(ids.numel(), D, dtype=torch.float32, device=table.device)
    lib.call("mhr_l2norm_rows_indexed_bwd", dy.data_ptr(), table.data_ptr(), table.shape[0], ids.data_ptr(), norms.data_ptr(),
             dx.data_ptr(), ids.numel(), D, _stream())
    return dx


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
def rows_gemm_supported(M, N, K, w_is_kn=False):
    return K in (64, 128, 256) and N > 0 and N % (256 if w_is_kn else 8) == 0 and M > 0          # (= mhr_rows_gemm_supported)


def rows_gemm(a, w, bias=None, out=None, w_is_kn=False):
    """out [M, N] bf16 = a [M, K] @ w.T (w [N, K]; w_is_kn: a @ w with w [K, N]) (+ bias [N] bf16): the encoder's token-rows
    projections (hstu.py:236-239, 281-288) with the weight stationary in registers and the token rows streaming through LDS."""
    for t_, nm in ((a, "a"), (w, "w")):                       # (rows may be a column block of a wider buffer: row strides are passed on)
        if not (t_.is_cuda and t_.dtype == torch.bfloat16 and t_.dim() == 2 and t_.stride(1) == 1):
            raise ValueError(f"rows_gemm: {nm} must be a 2-d bf16 device tensor with unit inner stride")
    M, K = a.shape
    N = w.shape[1] if w_is_kn else w.shape[0]
    if (w.shape[0] if w_is_kn else w.shape[1]) != K:
        raise ValueError("rows_gemm: inner dimensions differ")
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    elif out.shape != (M, N) or out.dtype != torch.bfloat16 or out.stride(1) != 1:
        raise ValueError("rows_gemm: out must be [M, N] bf16 with unit inner stride")
    if bias is not None:
        _chk(bias, "bias", torch.bfloat16)
    _timed_call("mhr_rows_gemm", a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), 1 if w_is_kn else 0,
                bias.data_ptr() if bias is not None else 0, out.data_ptr(), out.stride(0), M, N, K, _stream())
    return out


def rows_gemm_deep_supported(M, N, K, w_is_kn=False):
    return K == 1024 and N > 0 and N % 128 == 0 and M > 0                                        # (= mhr_rows_gemm_deep_supported)


def rows_gemm_deep(a, w, out=None, w_is_kn=False):
    """out [M, N] bf16 = a [M, 1024] @ w.T (w [N, 1024]; w_is_kn: a @ w with w [1024, N]): the input gradients of the uvqk
    projection and of the decoding heads (the autograd of hstu.py:236-239 and of llm_heads.py's linears under bf16 autocast),
    with the whole K = 1024 of a wave's 32 output columns stationary in registers and the token rows streaming through LDS."""
    for t_, nm in ((a, "a"), (w, "w")):                       # (rows may be a column block of a wider buffer: row strides are passed on)
        if not (t_.is_cuda and t_.dtype == torch.bfloat16 and t_.dim() == 2 and t_.stride(1) == 1):
            raise ValueError(f"rows_gemm_deep: {nm} must be a 2-d bf16 device tensor with unit inner stride")
    M, K = a.shape
    N = w.shape[1] if w_is_kn else w.shape[0]
    if (w.shape[0] if w_is_kn else w.shape[1]) != K:
        raise ValueError("rows_gemm_deep: inner dimensions differ")
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    elif out.shape != (M, N) or out.dtype != torch.bfloat16 or out.stride(1) != 1:
        raise ValueError("rows_gemm_deep: out must be [M, N] bf16 with unit inner stride")
    _timed_call("mhr_rows_gemm_deep", a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), 1 if w_is_kn else 0,
                out.data_ptr(), out.stride(0), M, N, K, _stream())
    return out


def seq_pack_maps(key_valid, B, L, capacity, guard=None):
    """(cu_rows [B+1], src_of [capacity], row_of [B*L], overflow [1]) int32 of a batch of masks (mhr_seq_pack_maps).
    guard (int32 [4] device tensor of the caller, zeroed once): the same maps through mhr_seq_pack_maps_guarded, which also
    records an overflow in those words - (overflowing calls, largest count, its capacity, 0) - and never clears them."""
    _chk(key_valid, "key_valid", torch.uint8)
    dev = key_valid.device
    cu = torch.empty(B + 1, dtype=torch.int32, device=dev)
    src_of = torch.empty(capacity, dtype=torch.int32, device=dev)
    row_of = torch.empty(B * L, dtype=torch.int32, device=dev)
    overflow = torch.empty(1, dtype=torch.int32, device=dev)
    if guard is None:
        lib.call("mhr_seq_pack_maps", key_valid.data_ptr(), B, L, int(capacity), cu.data_ptr(), src_of.data_ptr(), row_of.data_ptr(),
                 overflow.data_ptr(), _stream())
    else:
        _chk(guard, "guard", torch.int32)
        if guard.numel() != 4 or guard.device != dev:
            raise ValueError("seq_pack_maps: guard must be int32 [4] on the mask's device")
        lib.call("mhr_seq_pack_maps_guarded", key_valid.data_ptr(), B, L, int(capacity), cu.data_ptr(), src_of.data_ptr(),
                 row_of.data_ptr(), overflow.data_ptr(), guard.data_ptr(), _stream())
    return cu, src_of, row_of, overflow


def rows_gather_masked(src, idx, out=None):
    """out[r] = src[idx[r]] where idx[r] >= 0, zeros elsewhere (rows of f32 or bf16; idx int32)."""
    _chk(src, "src")
    _chk(idx, "idx", torch.int32)
    n, dim = idx.numel(), src.shape[-1]
    if out is None:
        out = torch.empty(n, dim, dtype=src.dtype, device=src.device)
    lib.call("mhr_rows_gather_masked", src.data_ptr(), _dt(src), idx.data_ptr(), out.data_ptr(), n, dim, _stream())
    return out


PACK_ROWS = os.environ.get("MHR_PACK_ROWS", "1") != "0"          # encoder over the valid rows only when the batch carries a row capacity
PACK_HEADS = os.environ.get("MHR_PACK_HEADS", "1") != "0"        # ... and the embedding gather, the decoding heads and the loss with it: no window-shaped activation in a train step
DEAD_ROWS = os.environ.get("MHR_DEAD_ROWS", "1") != "0"          # row-wise encoder kernels do not load rows in front of a sequence's first valid key
SEQ_LAYOUT = os.environ.get("MHR_ATTN_SEQ_LAYOUT", "1") != "0"   # skip leading all-padding blocks + longest-sequences-first launch order


def attn_seq_layout(key_valid, B, L, order=True):
    """(first_block [B] int32, seq_order [B] int32 | None, first_row [B] int32) of a batch of masks: the 32-row block holding each
    sequence's first valid key, the sequences ordered by it (most live blocks first), and the index of that key (L when none).
    Computed once per batch, read by every layer's attention launches (`layout=` of hstu_attn_fwd / hstu_attn_bwd) and row-wise
    kernels (`dead=(first_row, L)`)."""
    _chk(key_valid, "key_valid", torch.uint8)
    first = torch.empty(B, dtype=torch.int32, device=key_valid.device)
    first_row = torch.empty(B, dtype=torch.int32, device=key_valid.device)
    order_t = torch.empty(B, dtype=torch.int32, device=key_valid.device) if order else None
    lib.call("mhr_attn_seq_layout", key_valid.data_ptr(), B, L, first.data_ptr(), order_t.data_ptr() if order else 0,
             first_row.data_ptr(), _stream())
    return first, order_t, first_row


def _layout_ptrs(layout):
    """(first_block, seq_order, cu_rows) pointers of a layout tuple (first_block | None, seq_order | None, first_row, cu_rows)."""
    if layout is None:
        return 0, 0, 0
    first, order = layout[0], layout[1]
    cu = layout[3] if len(layout) > 3 else None
    return (first.data_ptr() if first is not None else 0), (order.data_ptr() if order is not None else 0), (cu.data_ptr() if cu is not None else 0)


def hstu_attn_fwd(h, key_valid, B, L, n_heads, head_dim, apply_silu=True, save_act=True, layout=None):
    """h [B*L, 4*D] bf16 pre-activation uvqk (column blocks u|v|q|k).  Returns (out [B*L, D], act [B*L, 3*D] (q|k|v))."""
    _chk(h, "h", torch.bfloat16)
    _chk(key_valid, "key_valid", torch.uint8)
    D = n_heads * head_dim
    stride = h.stride(0)
    esz = 2
    base = h.data_ptr()
    v_ptr, q_ptr, k_ptr = base + D * esz, base + 2 * D * esz, base + 3 * D * esz
    R = h.shape[0]                               # B * L windows, or the capacity of a packed batch (layout[3] = cu_rows)
    out = torch.empty(R, D, dtype=torch.bfloat16, device=h.device)
    act = torch.empty(R, 3 * D, dtype=torch.bfloat16, device=h.device) if save_act else None
    aq = act.data_ptr() if save_act else 0
    fb, so, cu = _layout_ptrs(layout)
    _timed_call("mhr_hstu_attn_fwd_seq", q_ptr, k_ptr, v_ptr, stride, key_valid.data_ptr(), out.data_ptr(),
             aq, aq + D * esz if save_act else 0, aq + 2 * D * esz if save_act else 0, 3 * D,
             B, L, n_heads, head_dim, 1 if apply_silu else 0, fb, so, cu, R if cu else 0, _stream())
    return out, act


def hstu_attn_bwd(h, act, key_valid, d_out, dh, B, L, n_heads, head_dim, apply_silu=True, layout=None):
    """writes dv|dq|dk into dh[:, D:4D] (pre-activation gradients).  act = None: the activated q / k / v are recomputed
    from h inside the kernel (apply_silu only)."""
    D = n_heads * head_dim
    esz = 2
    base, dbase = h.data_ptr(), dh.data_ptr()
    abase = act.data_ptr() if act is not None else 0
    fb, so, cu = _layout_ptrs(layout)
    _timed_call("mhr_hstu_attn_bwd_seq", base + 2 * D * esz, base + 3 * D * esz, base + D * esz, h.stride(0),
             abase, abase + D * esz if act is not None else 0, abase + 2 * D * esz if act is not None else 0,
             act.stride(0) if act is not None else 0, key_valid.data_ptr(), d_out.data_ptr(),
             dbase + 2 * D * esz, dbase + 3 * D * esz, dbase + D * esz, dh.stride(0),
             B, L, n_heads, head_dim, 1 if apply_silu else 0, fb, so, cu, h.shape[0] if cu else 0, _stream())
    return dh


# ------------------------------------------------------------------------------------------------
# LLM decoder blocks (HLLM twin): RMSNorm, SwiGLU, RoPE, causal softmax attention
# ------------------------------------------------------------------------------------------------
def rmsnorm_fwd(x, weight, res=None, eps=1e-6):
    """x f32 [rows, D] (+ res bf16) -> (x_out f32 (x itself without res), y bf16, rstd f32 [rows])."""
    _chk(x, "x", torch.float32)
    _chk(weight, "weight", torch.float32)
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    x_out = x
    if res is not None:
        _chk(res, "res", torch.bfloat16)
        x_out = torch.empty_like(x)
    _timed_call("mhr_rmsnorm_fwd", x.data_ptr(), _ptr(res), weight.data_ptr(), x_out.data_ptr(), y.data_ptr(), rstd.data_ptr(),
                rows, D, float(eps), _stream())
    return x_out, y, rstd


def rmsnorm_bwd(dy, x_out, weight, rstd, d_xout=None, want_dres=False):
    """-> (dx f32, dres bf16 or None, dw f32 [D])."""
    _chk(dy, "dy", torch.bfloat16)
    _chk(x_out, "x_out", torch.float32)
    D = x_out.shape[-1]
    rows = x_out.numel() // D
    dx = torch.empty_like(x_out)
    dres = torch.empty(x_out.shape, dtype=torch.bfloat16, device=x_out.device) if want_dres else None
    parts = lib.load().mhr_rmsnorm_bwd_parts(rows)
    dw_part = torch.empty(parts, D, dtype=torch.float32, device=x_out.device)
    if d_xout is not None:
        _chk(d_xout, "d_xout", torch.float32)
    _timed_call("mhr_rmsnorm_bwd", dy.data_ptr(), x_out.data_ptr(), weight.data_ptr(), rstd.data_ptr(), _ptr(d_xout),
                dx.data_ptr(), _ptr(dres), dw_part.data_ptr(), rows, D, _stream())
    return dx, dres, dw_part.sum(0)


def swiglu_fwd(gate_up):
    _chk(gate_up, "gate_up", torch.bfloat16)
    F2 = gate_up.shape[-1]
    rows = gate_up.numel() // F2
    act = torch.empty(*gate_up.shape[:-1], F2 // 2, dtype=torch.bfloat16, device=gate_up.device)
    _timed_call("mhr_swiglu_fwd", gate_up.data_ptr(), act.data_ptr(), rows, F2 // 2, _stream())
    return act


def swiglu_bwd(gate_up, d_act):
    _chk(gate_up, "gate_up", torch.bfloat16)
    _chk(d_act, "d_act", torch.bfloat16)
    F2 = gate_up.shape[-1]
    rows = gate_up.numel() // F2
    d = torch.empty_like(gate_up)
    _timed_call("mhr_swiglu_bwd", gate_up.data_ptr(), d_act.data_ptr(), d.data_ptr(), rows, F2 // 2, _stream())
    return d


def rope_inplace(x, n_heads, head_dim, cos, sin, positions=None, seq_len=0, inverse=False):
    """Rotate the first n_heads heads of every row of x [T, stride] bf16 in place."""
    _chk(x, "x", torch.bfloat16)
    _chk(cos, "cos", torch.float32)
    _chk(sin, "sin", torch.float32)
    if positions is not None:
        _chk(positions, "positions", torch.int32)
    assert cos.shape == sin.shape and cos.shape[1] == head_dim // 2 and n_heads * head_dim <= x.shape[-1]
    T = x.numel() // x.shape[-1]
    _timed_call("mhr_rope_inplace", x.data_ptr(), x.shape[-1], _ptr(positions), cos.data_ptr(), sin.data_ptr(), T, int(seq_len),
                n_heads, head_dim, cos.shape[0], 1 if inverse else 0, _stream())
    return x


def softmax_attn_fwd(qkv, n_seqs, max_len, n_heads, n_kv_heads, head_dim, scale, cu_seqlens=None, key_valid=None):
    """qkv [T, (n_heads + 2 n_kv_heads) * head_dim] bf16 (q | k | v column blocks) -> (out [T, n_heads*head_dim] bf16, lse)."""
    _chk(qkv, "qkv", torch.bfloat16)
    T, stride = qkv.shape
    assert stride == (n_heads + 2 * n_kv_heads) * head_dim
    if cu_seqlens is not None:
        _chk(cu_seqlens, "cu_seqlens", torch.int32)
        assert cu_seqlens.numel() == n_seqs + 1
    else:
        assert T == n_seqs * max_len
    if key_valid is not None:
        _chk(key_valid, "key_valid", torch.uint8)
        assert key_valid.numel() == T
    out = torch.empty(T, n_heads * head_dim, dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty(T, n_heads, dtype=torch.float32, device=qkv.device)
    e = qkv.element_size()
    q, k = qkv.data_ptr(), qkv.data_ptr() + n_heads * head_dim * e
    v = k + n_kv_heads * head_dim * e
    _timed_call("mhr_softmax_attn_fwd", q, k, v, stride, _ptr(cu_seqlens), _ptr(key_valid), out.data_ptr(), lse.data_ptr(),
                n_seqs, max_len, n_heads, n_kv_heads, head_dim, float(scale), _stream())
    return out, lse


def softmax_attn_bwd(qkv, out, d_out, lse, n_seqs, max_len, n_heads, n_kv_heads, head_dim, scale, cu_seqlens=None,
                     key_valid=None):
    """-> dqkv [T, (n_heads + 2 n_kv_heads) * head_dim] bf16 (KV-head gradients summed over their query-head group in fp32)."""
    _chk(qkv, "qkv", torch.bfloat16)
    _chk(out, "out", torch.bfloat16)
    _chk(d_out, "d_out", torch.bfloat16)
    T, stride = qkv.shape
    dqkv = torch.empty_like(qkv)
    e = qkv.element_size()
    q, k = qkv.data_ptr(), qkv.data_ptr() + n_heads * head_dim * e
    v = k + n_kv_heads * head_dim * e
    group = n_heads // n_kv_heads
    if group == 1:
        dk_ptr = dqkv.data_ptr() + n_heads * head_dim * e
        dv_ptr = dk_ptr + n_kv_heads * head_dim * e
        dkv_stride, slabs = stride, None
    else:
        slabs = torch.empty(2, T, n_heads * head_dim, dtype=torch.bfloat16, device=qkv.device)
        dk_ptr, dv_ptr, dkv_stride = slabs[0].data_ptr(), slabs[1].data_ptr(), n_heads * head_dim
    _timed_call("mhr_softmax_attn_bwd", q, k, v, stride, _ptr(cu_seqlens), _ptr(key_valid), out.data_ptr(), d_out.data_ptr(),
                lse.data_ptr(), dqkv.data_ptr(), stride, dk_ptr, dv_ptr, dkv_stride, n_seqs, max_len, n_heads, n_kv_heads,
                head_dim, float(scale), _stream())
    if slabs is not None:
        red = torch.sum(slabs.view(2, T, n_kv_heads, group, head_dim), dim=3, dtype=torch.float32)      # [2, T, n_kv, hd]
        dqkv[:, n_heads * head_dim:].view(T, 2, n_kv_heads * head_dim).copy_(red.view(2, T, -1).transpose(0, 1))
    return dqkv


# ------------------------------------------------------------------------------------------------
# sampled softmax
# ------------------------------------------------------------------------------------------------
def token_compact(mask, q_all, p_all, o_all, tok_cap=None, slot_map=False, packed=None):
    """Ordered compaction of live (group, slot) pairs.  mask [G, n_slots] bool/uint8 (any nonzero byte is live); q_all [G, n_slots] int32;
    p_all, o_all [n_slots] int32.  Returns (q_idx, p_idx, o_idx [G, cap] int32 - entries beyond n_tok undefined -,
    n_tok [G] int32) with cap = tok_cap (default n_slots) rounded up to a multiple of 32.  No host sync.
    slot_map: also return tok_of_slot [G, n_slots] int32 (list position of a live slot, -1 otherwise).
    packed = (row_of, seq_len, n_heads, head_stride): q_all holds the window form (b H + h) L + l and q_idx receives the PACKED
    head row h * head_stride + row_of[b L + l] (head rows [H, head_stride, D] over seq_pack_maps' rows); everything else as before."""
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    _chk(mask, "mask", torch.uint8)
    _chk(q_all, "q_all", torch.int32)
    _chk(p_all, "p_all", torch.int32)
    _chk(o_all, "o_all", torch.int32)
    G, n_slots = mask.shape
    assert q_all.shape == (G, n_slots) and p_all.numel() == n_slots and o_all.numel() == n_slots
    cap = ((n_slots if tok_cap is None else tok_cap) + 31) // 32 * 32
    dev = mask.device
    q_idx = torch.empty(G, cap, dtype=torch.int32, device=dev)
    p_idx = torch.empty(G, cap, dtype=torch.int32, device=dev)
    o_idx = torch.empty(G, cap, dtype=torch.int32, device=dev)
    n_tok = torch.empty(G, dtype=torch.int32, device=dev)
    scratch = torch.empty(G, (n_slots + 4095) // 4096, dtype=torch.int32, device=dev)
    tos = torch.empty(G, n_slots, dtype=torch.int32, device=dev) if slot_map else None
    row_of, seq_len, n_heads, head_stride = packed if packed is not None else (None, 0, 0, 0)
    if row_of is not None:
        _chk(row_of, "row_of", torch.int32)
    lib.call("mhr_token_compact", mask.data_ptr(), q_all.data_ptr(), p_all.data_ptr(), o_all.data_ptr(), G, n_slots, cap,
             q_idx.data_ptr(), p_idx.data_ptr(), o_idx.data_ptr(), n_tok.data_ptr(), scratch.data_ptr(), _ptr(tos),
             _ptr(row_of), int(seq_len), int(n_heads), int(head_stride), _stream())
    if slot_map:
        return q_idx, p_idx, o_idx, n_tok, tos
    return q_idx, p_idx, o_idx, n_tok


def loss_reduce(bucket_sum, bucket_cnt, weight, n_segments):
    """[G,P] per-offset loss sums / token counts / weights -> (total [], flat [G P + G S + G + S] = per_gp | seg_all | g_tot | seg_sum)
    (mhr_loss_reduce: one launch for the mean, the weighting and every logged partial sum)."""
    for t, n in ((bucket_sum, "bucket_sum"), (bucket_cnt, "bucket_cnt"), (weight, "weight")):
        _chk(t, n, torch.float32)
    G, P = bucket_sum.shape
    assert bucket_cnt.shape == (G, P) and weight.shape == (G, P) and P % n_segments == 0
    total = torch.empty((), dtype=torch.float32, device=bucket_sum.device)
    out = torch.empty(G * P + G * n_segments + G + n_segments, dtype=torch.float32, device=bucket_sum.device)
    lib.call("mhr_loss_reduce", bucket_sum.data_ptr(), bucket_cnt.data_ptr(), weight.data_ptr(), G, P, int(n_segments),
             total.data_ptr(), out.data_ptr(), _stream())
    return total, out


def loss_reduce_bwd(d_total, bucket_cnt, weight):
    """Token weight per (group, offset) bucket for the backward kernels: d_total * weight / max(cnt, 1)."""
    d_total = d_total.reshape(1).float().contiguous()
    w = torch.empty_like(weight)
    lib.call("mhr_loss_reduce_bwd", d_total.data_ptr(), bucket_cnt.data_ptr(), weight.data_ptr(), weight.numel(), w.data_ptr(), _stream())
    return w


def nce_log_counters(n_valid, rank, o_idx, n_tok_dev, group, ks):
    """-> f32 [1 + len(ks)]: mean n_valid and mean(rank < k) over the live offset-0 tokens of `group` (hstu.py:621-629)."""
    import ctypes
    G, cap = o_idx.shape
    for t in (n_valid, rank, o_idx):
        _chk(t, "nce_log_counters input", torch.int32) if t.is_contiguous() else None
        assert t.shape == (G, cap) and t.stride(0) == t.shape[1] * t.stride(1) or t.is_contiguous(), "token tables must share one [G, cap] layout"
        assert t.stride(0) == cap and t.stride(1) == 1 and t.dtype == torch.int32
    out = torch.empty(1 + len(ks), dtype=torch.float32, device=o_idx.device)
    ks_arr = (ctypes.c_int32 * max(1, len(ks)))(*ks)
    key = str(o_idx.device)
    if key not in _COUNTER_SCRATCH:       # self-cleaning (the kernel zeroes it again), one per device, never freed: graph-safe
        _COUNTER_SCRATCH[key] = torch.zeros(8, dtype=torch.int64, device=o_idx.device)
    lib.call("mhr_nce_log_counters", n_valid.data_ptr(), rank.data_ptr(), o_idx.data_ptr(), n_tok_dev.data_ptr(), int(group), cap,
             ctypes.addressof(ks_arr), len(ks), _COUNTER_SCRATCH[key].data_ptr(), out.data_ptr(), _stream())
    return out


_COUNTER_SCRATCH = {}
STREAM_DIMS = (16, 32, 64, 128, 256)      # feature dims of the register-stationary streaming kernels
FILTER_FALSE_NEGATIVE_TEST = os.environ.get("MHR_NCE_FIX_FILTER", "1") != "0"    # 0: the exhaustive bit-table kernel
SHARE_ROWS = os.environ.get("MHR_NCE_SHARE_ROWS", "1") != "0"
DETERMINISTIC = False
_ROW_IOTA = {}
_ZERO_FIX = {}


def nce_path(dim, share_rows, ihn_beta=0.0):
    """The path a sampled-softmax call takes: "wide" (wide.py) for feature dims beyond the register-stationary kernels and for the
    IHN loss at every dim; "shared" (query-row sharing) where the caller asks for it and SHARE_ROWS allows it; else "tokens"."""
    if dim not in STREAM_DIMS or float(ihn_beta) > 0:
        return "wide"
    return "shared" if share_rows and SHARE_ROWS else "tokens"


class NceSaved:
    """What the sampled-softmax forward keeps for the backward: here the fields every path has ([G, cap] tensors at token
    capacity), one subclass per path (nce_path) for the rest.  Every field is given once, to the constructor."""
    __slots__ = ("q_idx", "p_idx", "n_tok_dev", "tok_cap", "cap", "groups", "dim", "n_neg", "thres", "negs",
                 "loss", "lse", "s_pos", "n_valid", "rank", "bucket_idx", "n_buckets", "bucket_sum", "bucket_cnt")
    shared = wide = False

    def __init__(self, loss, n_valid, rank, **fields):
        tc = fields["tok_cap"]              # loss / n_valid / rank arrive as the [G, cap] buffers the kernels wrote: cut here, once
        fields.update((k, None if t is None else t[:, :tc]) for k, t in (("loss", loss), ("n_valid", n_valid), ("rank", rank)))
        names = {n for c in type(self).__mro__ for n in getattr(c, "__slots__", ())}
        assert names == set(fields), (type(self).__name__, sorted(names ^ set(fields)))
        for n, v in fields.items():
            setattr(self, n, v)


class NceSavedTokens(NceSaved):
    """Per-token streaming kernels (csrc/nce.hip): everything [G, cap, ...]; u: the unnormalised token-side gradient."""
    __slots__ = ("qn", "pn", "q_inv", "p_inv", "u", "supp")


class NceSavedShared(NceSaved):
    """Query-row sharing (csrc/nce_shared.hip): row-level state of the streaming kernels + the maps between rows and tokens."""
    __slots__ = ("qn", "u", "q_inv", "supp", "pn", "p_inv",   # per distinct query ROW (supp: None for whole-tile pools) / TARGET row
                 "tok2row", "row_first", "row_q", "n_row_dev", "row_cap", "fix_words", "fix_slot", "fix_any", "n_p_rows",
                 "window",                                # (tok_of_slot [G, n_slots], L, P) of window-structured lists, or None
                 "bwd_bufs")                              # (dq, dp, d_negs, d_scale, lw_row) zeroed by an early prep, or None
    shared = True

    def take_bwd_bufs(self):                              # one backward may accumulate into them
        bufs, self.bwd_bufs = self.bwd_bufs, None
        return bufs


class NceSavedWide(NceSaved):
    """Wide / dense path (wide.py): qn .. p_inv per token; wide_pack: per group the packed negatives + suppression bits of the
    hand-written contraction (None: dense chunks); REMI's interest-aware hard-negative loss: beta and the two saved log-sums per token."""
    __slots__ = ("qn", "pn", "q_inv", "p_inv", "scale_dev", "cap_eff", "wide_pack", "ihn_beta", "ihn_num", "ihn_imp")
    wide = True


def set_deterministic(on):
    """Order-independent reductions in the loss backward (include/mhr.h: deterministic mode): fixed-point accumulators for the
    negative-side gradient, ordered partial sums for d(logit_scale), single-range column sums, a fixed-order fold of the per-offset
    loss sums.  Bitwise reproducible steps (run to run, replayed vs host-issued) for the row-sharing sampled softmax (loss =
    'prior' with pred_len > 1: cfg1); a few per cent slower.  Process-wide; also MHR_DETERMINISTIC=1 in the environment."""
    global DETERMINISTIC
    DETERMINISTIC = bool(on)
    lib.call("mhr_set_deterministic", 1 if on else 0)


if os.environ.get("MHR_DETERMINISTIC", "0") == "1":
    try:
        set_deterministic(True)
    except RuntimeError:          # (library not built yet: lib.load() raises at the first real use anyway)
        DETERMINISTIC = True


def _row_maps(q_idx, n_tok_dev, cap, row_cap):
    """Runs of equal query rows in the (offset-fastest) token lists -> (row list [G, row_cap], tok2row [G, cap],
    row_first [G, row_cap], n_row [G]); all on the device, no host sync (mhr_row_maps: count + scan, like the compaction)."""
    G = q_idx.shape[0]
    dev = q_idx.device
    r_q, r_first = zeros_many(dev, ((G, row_cap), torch.int32), ((G, row_cap), torch.int32))
    tok2row = torch.empty(G, cap, dtype=torch.int32, device=dev)
    n_row = torch.empty(G, dtype=torch.int32, device=dev)
    scratch = torch.empty(G, (cap + 4095) // 4096, dtype=torch.int32, device=dev)
    lib.call("mhr_row_maps", q_idx.data_ptr(), n_tok_dev.data_ptr(), G, cap, row_cap, r_q.data_ptr(), r_first.data_ptr(),
             tok2row.data_ptr(), n_row.data_ptr(), scratch.data_ptr(), _stream())
    return r_q, tok2row, r_first, n_row


def _fix_table_geometry(p_rows, n_neg):
    """(n_p_rows, rp_pad, n_tiles) of the bit table [G, n_tiles, rp_pad]: a column per target row (256-row blocks), a word per 32 negatives."""
    return p_rows.shape[0], (p_rows.shape[0] + 255) // 256 * 256, (n_neg + 31) // 32


def _p_row_lists(p_row_mask, G, n_p_rows, rp_pad, slot_of_row=None):
    """p_row_mask [G, n_p_rows] -> (row_list [G, rp_pad], n_list [G], slot_of_row [G, n_p_rows]), all None without a mask: per group
    the rows of p_rows the mask names, compacted on the device.  The bit-table kernels test only those rows (slot j of the list = column
    j of the table) and write the inverse map themselves, into slot_of_row: the caller's or a new one (zero: any lookup stays in bounds)."""
    if p_row_mask is None:
        return None, None, None
    assert p_row_mask.shape == (G, n_p_rows)
    dev = p_row_mask.device
    key = (G, n_p_rows, str(dev))
    if key not in _ROW_IOTA:
        ar = torch.arange(n_p_rows, dtype=torch.int32, device=dev)
        _ROW_IOTA[key] = (ar[None].expand(G, -1).contiguous(), ar)
    iota_g, iota = _ROW_IOTA[key]
    row_list, _, _, n_list = token_compact(p_row_mask.contiguous(), iota_g, iota, iota, tok_cap=rp_pad)
    return row_list, n_list, torch.zeros(G, n_p_rows, dtype=torch.int32, device=dev) if slot_of_row is None else slot_of_row


def _fix_bits_launch(p_rows, negs, n_neg, D, G, thres, p_row_mask):
    """The false-negative bit table of the target rows, for the row-sharing path: (fix_words, fix_any, slot_of_row)."""
    dev = negs.device
    n_p_rows, rp_pad, n_tiles = _fix_table_geometry(p_rows, n_neg)
    fix_words = torch.empty(G, n_tiles, rp_pad, dtype=torch.int32, device=dev)
    fix_any, slot_of_row = zeros_many(dev, ((G, rp_pad), torch.int32), ((G, n_p_rows), torch.int32))
    row_list, n_list, slot_of_row = _p_row_lists(p_row_mask, G, n_p_rows, rp_pad, slot_of_row)
    if FILTER_FALSE_NEGATIVE_TEST and D >= 128:
        # prefix filter + exact pass over the survivors (same table, bit for bit); smaller dims keep the exhaustive kernel
        ws_bytes = lib.load().mhr_nce_fix_bits_filtered_workspace_bytes(n_p_rows, n_neg, G)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        lib.call("mhr_nce_fix_bits_filtered", p_rows.data_ptr(), _dt(p_rows), n_p_rows, negs.data_ptr(), n_neg, D, G, float(thres),
                 fix_words.data_ptr(), _ptr(row_list), _ptr(n_list), _ptr(slot_of_row), fix_any.data_ptr(), ws.data_ptr(), ws_bytes,
                 _stream())
    else:
        lib.call("mhr_nce_fix_bits", p_rows.data_ptr(), _dt(p_rows), n_p_rows, negs.data_ptr(), n_neg, D, G, float(thres),
                 fix_words.data_ptr(), _ptr(row_list), _ptr(n_list), _ptr(slot_of_row), fix_any.data_ptr(), _stream())
    return fix_words, fix_any, slot_of_row


class NcePrep:
    """The batch-only half of the row-sharing forward; the stages of `nce_shared_prepare_stages` fill it in order."""
    __slots__ = ("key", "keep",                                        # _prep_key of the call it serves; those inputs, kept alive
                 "row_q", "tok2row", "row_first", "n_row", "r_p",     # _row_maps of the lists; the target of every row's first token
                 "fix_words", "fix_any", "slot_of_row",               # _fix_bits_launch: the bit table of the target rows
                 "sum_row", "nv_row", "rk_row", "n_valid", "rank",    # zeroed: per row / per token (counters: None without logs)
                 "pn_rows", "p_inv", "bwd")       # normalised target rows; (dq, dp, d_negs, d_scale, lw_row) with n_q_rows, else None


def _prep_key(q_idx, p_idx, p_rows, negs, thres, want_logs):
    return (q_idx.data_ptr(), p_idx.data_ptr(), p_rows.data_ptr(), negs.data_ptr(), float(thres), bool(want_logs))


def nce_shared_prepare_stages(q_idx, p_idx, n_tok_dev, p_rows, negs, thres, p_row_mask, want_logs, n_q_rows=None):
    """Everything the row-sharing forward needs that depends on the BATCH only (token lists, target rows, negatives) and not
    on the query rows: the row maps of the token lists, the false-negative bit table of the target rows, the first target of
    every row, the normalised target rows and the zeroed accumulators (with n_q_rows, the number of query rows, the backward's
    accumulators as well).  `nce_fwd(share_rows=True)` builds it itself; a model may build it EARLY - on a second stream
    underneath the sequence encoder, a stage at a time between the encoder's layers - and hand it in (`prep=`).
    Returns (prep, stages): the NcePrep the stages fill, and the stages (callables, to be run in order on one stream); (None, [])
    when the shapes are not the row-sharing path's (ragged capacity / pool sizes, feature dims it does not take)."""
    cap, n_neg, D = q_idx.shape[1], negs.shape[1], negs.shape[2]
    # whole tiles only: nce_fwd pads a ragged capacity or pool into NEW tensors, which an early prep cannot have been built for
    if nce_path(D, True) != "shared" or cap % 32 or n_neg % 32:
        return None, []
    return _shared_prepare_stages(q_idx, p_idx, n_tok_dev, p_rows, negs, n_neg, thres, p_row_mask, want_logs, n_q_rows)


def _shared_prepare_stages(q_idx, p_idx, n_tok_dev, p_rows, negs, n_neg, thres, p_row_mask, want_logs, n_q_rows=None):
    """(n_neg: the pool's own size; `negs` may be padded to whole 32-row tiles behind it)"""
    (G, cap), D, dev = q_idx.shape, negs.shape[2], negs.device
    row_cap = cap + 32
    prep = NcePrep()
    prep.key, prep.keep, prep.bwd = _prep_key(q_idx, p_idx, p_rows, negs, thres, want_logs), (q_idx, p_idx, p_rows, negs), None

    def row_maps():
        prep.row_q, prep.tok2row, prep.row_first, prep.n_row = _row_maps(q_idx, n_tok_dev, cap, row_cap)

    def fix_bits():                 # the real false-negative bit table, per target row
        prep.fix_words, prep.fix_any, prep.slot_of_row = _fix_bits_launch(p_rows, negs, n_neg, D, G, thres, p_row_mask)

    def rows_and_zeros():
        prep.r_p = torch.gather(p_idx, 1, prep.row_first.long().clamp_(max=cap - 1)).contiguous()
        z = zeros_many(dev, ((G, row_cap), torch.float32), ((G, row_cap), torch.int32), ((G, row_cap), torch.int32),
                       ((G, cap), torch.int32), ((G, cap), torch.int32))
        prep.sum_row, prep.nv_row, prep.rk_row, prep.n_valid, prep.rank = z if want_logs else (z[0], None, None, None, None)
        # the normalised target is a property of the TARGET ROW (shared by every token and group that points at it)
        prep.pn_rows, p_norm = l2norm_rows(p_rows.contiguous(), torch.bfloat16, want_norms=True)
        prep.p_inv = 1.0 / p_norm

    def backward_buffers():         # zero / +inf fills that wait for nothing: (dq, dp, d_negs, d_scale, lw_row)
        dq, dp, dn, dls = zeros_many(dev, ((int(n_q_rows), D), torch.float32), ((p_rows.shape[0], D), torch.float32),
                                     ((G, n_neg, D), torch.float32), ((1,), torch.float32))
        prep.bwd = (dq, dp, dn, dls, torch.full((G, row_cap), float("inf"), dtype=torch.float32, device=dev))

    return prep, [row_maps, fix_bits, rows_and_zeros] + ([backward_buffers] if n_q_rows is not None else [])


def nce_shared_prepare(q_idx, p_idx, n_tok_dev, p_rows, negs, thres, p_row_mask, want_logs, n_q_rows=None):
    """`nce_shared_prepare_stages` run in one go on the current stream: the finished prep (or None)."""
    prep, stages = nce_shared_prepare_stages(q_idx, p_idx, n_tok_dev, p_rows, negs, thres, p_row_mask, want_logs, n_q_rows)
    for f in stages:
        f()
    return prep


def _nce_fwd_shared(c, q_rows, p_rows, logit_scale, want_logs, log_group, p_row_mask, window, prep):
    """Query-row sharing (csrc/nce_shared.hip): the streaming kernels see each distinct query row once.  c: the record's common fields
    (n_neg: the pool's own size, negs is padded).  -> (record class, its own fields, the sums for mhr_nce_finalize, n_valid, rank)."""
    G, cap, D, n_neg, thres, dev = c.groups, c.cap, c.dim, c.n_neg, c.thres, c.negs.device
    q_idx, p_idx, negs, n_tok_dev, s_pos = c.q_idx, c.p_idx, c.negs, c.n_tok_dev, c.s_pos
    row_cap, st = cap + 32, _stream()
    n_p_rows, rp_pad, n_tiles = _fix_table_geometry(p_rows, n_neg)
    if prep is not None and prep.key != _prep_key(q_idx, p_idx, p_rows, negs, thres, want_logs):
        raise ValueError("nce_fwd: prep was built for other token lists / target rows / negatives than this call's")
    if prep is None:
        prep, stages = _shared_prepare_stages(q_idx, p_idx, n_tok_dev, p_rows, negs, n_neg, thres, p_row_mask, want_logs)
        for f in stages:
            f()
    # (1) prep.fix_words: the real false-negative bit table, per target row
    # (2) the fused streaming forward over the ROWS with NOTHING suppressed (mhr_nce_fwd's plain form: no bit table, no
    #     suppression words, no normalised-target rows written); its positive is the target of the row's first token, so the
    #     log counters of offset-0 tokens come out of this launch.  Pools that are not whole 32-negative tiles take the
    #     general form with an all-zero bit table that is never written.
    qn_row = torch.empty(G, row_cap, D, dtype=torch.bfloat16, device=dev)
    q_inv_row, p_inv_row, s_pos_row = (torch.empty(G, row_cap, dtype=torch.float32, device=dev) for _ in range(3))
    u_row = torch.empty(G, row_cap, D, dtype=torch.float32, device=dev)
    if n_neg % 32 == 0:
        pn_row = supp_row = None
        fix_args = (0, 0, 0, 0)
    else:
        zkey = (G, n_tiles, n_p_rows, str(dev))
        if zkey not in _ZERO_FIX:         # grow-only: a captured hipGraph of the step keeps reading the entry of its shape
            _ZERO_FIX[zkey] = (torch.zeros(G, n_tiles, rp_pad, dtype=torch.int32, device=dev),
                               torch.zeros(G, rp_pad, dtype=torch.int32, device=dev), torch.zeros(G, dtype=torch.int32, device=dev),
                               torch.zeros(G, n_p_rows, dtype=torch.int32, device=dev))
        fix_args = tuple(t.data_ptr() for t in _ZERO_FIX[zkey])
        pn_row = torch.empty(G, row_cap, D, dtype=torch.bfloat16, device=dev)
        supp_row = torch.empty(G, n_tiles, row_cap, dtype=torch.int32, device=dev)
    _timed_call("mhr_nce_fwd", q_rows.data_ptr(), prep.row_q.data_ptr(), p_rows.data_ptr(), prep.r_p.data_ptr(), _dt(q_rows),
                negs.data_ptr(), n_neg, D, G, prep.n_row.data_ptr(), row_cap, logit_scale.data_ptr(), float(thres),
                prep.sum_row.data_ptr(), _ptr(prep.nv_row), _ptr(prep.rk_row), qn_row.data_ptr(), _ptr(pn_row), _ptr(supp_row),
                q_inv_row.data_ptr(), p_inv_row.data_ptr(), s_pos_row.data_ptr(), int(log_group), u_row.data_ptr(), n_p_rows,
                *fix_args, st)
    # (3) per token: s+, sums and counters with the token's own suppressed negatives taken out, against prep.pn_rows (one
    #     l2norm pass over p_rows: the normalised target is a property of the TARGET ROW).  A half-wave per query row
    #     (mhr_nce_shared_fwd_rows: the per-token entry's values bit for bit), timed under the stage's name
    ssum = torch.empty(G, cap, dtype=torch.float32, device=dev)
    _timed_call("mhr_nce_shared_fwd_tokens", prep.pn_rows.data_ptr(), n_p_rows, p_idx.data_ptr(), prep.row_first.data_ptr(),
                prep.n_row.data_ptr(), G, cap, row_cap, qn_row.data_ptr(), prep.sum_row.data_ptr(), _ptr(prep.nv_row),
                _ptr(prep.rk_row), negs.data_ptr(), n_neg, D, logit_scale.data_ptr(), prep.fix_words.data_ptr(),
                _ptr(prep.slot_of_row), prep.fix_any.data_ptr(), s_pos.data_ptr(), ssum.data_ptr(), _ptr(prep.n_valid),
                _ptr(prep.rank), st, entry="mhr_nce_shared_fwd_rows")
    own = dict(qn=qn_row, u=u_row, q_inv=q_inv_row, supp=supp_row, pn=prep.pn_rows, p_inv=prep.p_inv, tok2row=prep.tok2row,
               row_first=prep.row_first, row_q=prep.row_q, n_row_dev=prep.n_row, row_cap=row_cap, fix_words=prep.fix_words,
               fix_slot=prep.slot_of_row, fix_any=prep.fix_any, n_p_rows=n_p_rows, window=window, bwd_bufs=prep.bwd)
    return NceSavedShared, own, ssum, prep.n_valid, prep.rank


def _nce_fwd_tokens(c, q_rows, p_rows, logit_scale, log_group, p_row_mask, n_valid, rank):
    """The per-token streaming kernels (csrc/nce.hip); arguments and result as for _nce_fwd_shared."""
    G, cap, D, n_neg, dev = c.groups, c.cap, c.dim, c.n_neg, c.negs.device
    n_p_rows, rp_pad, n_tiles = _fix_table_geometry(p_rows, n_neg)
    qn, pn = (torch.empty(G, cap, D, dtype=torch.bfloat16, device=dev) for _ in range(2))
    q_inv, p_inv = (torch.empty(G, cap, dtype=torch.float32, device=dev) for _ in range(2))
    supp = torch.empty(G, n_tiles, cap, dtype=torch.int32, device=dev)
    u = torch.empty(G, cap, D, dtype=torch.float32, device=dev)  # unnormalised token-side gradient (fused forward)
    ssum = torch.zeros(G, cap, dtype=torch.float32, device=dev)
    # hoisted form (mhr.h): the false-negative test runs once per (group, target row, negative) into a bit table.  The table is
    # the exhaustive one, built inside mhr_nce_fwd: the token kernel reads every word of it
    fix_words = torch.empty(G, n_tiles, rp_pad, dtype=torch.int32, device=dev)
    row_list, n_list, slot_of_row = _p_row_lists(p_row_mask, G, n_p_rows, rp_pad)
    _timed_call("mhr_nce_fwd", q_rows.data_ptr(), c.q_idx.data_ptr(), p_rows.data_ptr(), c.p_idx.data_ptr(), _dt(q_rows),
                c.negs.data_ptr(), n_neg, D, G, c.n_tok_dev.data_ptr(), cap, logit_scale.data_ptr(), c.thres,
                ssum.data_ptr(), _ptr(n_valid), _ptr(rank), qn.data_ptr(), pn.data_ptr(),
                supp.data_ptr(), q_inv.data_ptr(), p_inv.data_ptr(), c.s_pos.data_ptr(), int(log_group), u.data_ptr(),
                n_p_rows, fix_words.data_ptr(), _ptr(row_list), _ptr(n_list), _ptr(slot_of_row), _stream())
    return NceSavedTokens, dict(qn=qn, pn=pn, q_inv=q_inv, p_inv=p_inv, u=u, supp=supp), ssum, n_valid, rank


def nce_fwd(q_rows, q_idx, p_rows, p_idx, negs, n_tok_dev, tok_cap, logit_scale, thres=0.99, want_logs=False,
            bucket_idx=None, n_buckets=0, log_group=-1, p_row_mask=None, share_rows=False, window=None,
            ihn_beta=0.0, prep=None):
    """Grouped sampled softmax.  q_rows/p_rows [*, D] (bf16 or f32, same dtype, shared by all groups);
    q_idx/p_idx [G, tok_cap] int32; negs [G, n_neg, D] bf16 normalised; n_tok_dev [G] int32.
    (1-D q_idx / 2-D negs are accepted as a single group.)  Saved tensors carry the leading group axis.
    p_row_mask [G, p_rows.shape[0]] bool/uint8 (optional): per group, a superset of the rows of p_rows that live tokens
    point at - the hoisted false-negative test then visits only those rows.
    share_rows: tokens with the same query row are neighbours in the lists (several prediction offsets of one position):
    the negative-pool products run once per distinct row (csrc/nce_shared.hip).  Same results.
    window = (tok_of_slot, L, P) (with share_rows): the lists are the compaction of (b, l, p) window slots with
    p_idx = b (L + P) + l + 1 + p (token_compact(slot_map=True)): the backward then needs no per-token atomics.
    ihn_beta > 0: REMI's interest-aware hard-negative loss (remi.py:203-288) instead of the plain sampled softmax; runs on the
    dense path (library GEMM + the ihn_dense epilogues of csrc/wide.hip) at every feature dim.
    prep: `nce_shared_prepare(...)` of exactly these lists / rows / negatives, built earlier (row-sharing path only)."""
    if q_idx.dim() == 1:
        q_idx, p_idx, negs, n_tok_dev = q_idx[None], p_idx[None], negs[None], n_tok_dev.view(1)
    _chk(negs, "negs", torch.bfloat16)
    _chk(logit_scale, "logit_scale", torch.float32)
    for t, name in ((q_idx, "q_idx"), (p_idx, "p_idx"), (n_tok_dev, "n_tok_dev")):
        _chk(t, name, torch.int32)
    assert q_rows.dtype == p_rows.dtype
    dev = negs.device
    G, n_neg, D = negs.shape
    assert q_idx.shape == (G, tok_cap) and p_idx.shape == (G, tok_cap) and n_tok_dev.numel() == G
    if n_neg % 32:                                    # pools are stored [G, round_up(n_neg, 32), D]: whole tiles stream unclamped
        negs = torch.nn.functional.pad(negs, (0, 0, 0, 32 - n_neg % 32)).contiguous()
    # the kernels stream whole 32-token tiles: capacities are rounded up (production shapes already are multiples of 32)
    cap = (tok_cap + 31) // 32 * 32
    if cap != tok_cap:
        q_idx = torch.nn.functional.pad(q_idx, (0, cap - tok_cap)).contiguous()
        p_idx = torch.nn.functional.pad(p_idx, (0, cap - tok_cap)).contiguous()
        if bucket_idx is not None:
            bucket_idx = torch.nn.functional.pad(bucket_idx, (0, cap - tok_cap)).contiguous()
    if bucket_idx is not None:
        _chk(bucket_idx, "bucket_idx", torch.int32)
        assert bucket_idx.shape == (G, cap)
    path = nce_path(D, share_rows, ihn_beta)
    own_logs = want_logs and path != "shared"         # (the row-sharing path brings its own per-token counters)
    zf = zeros_many(dev, ((2, G, max(n_buckets, 1)), torch.float32), ((G, cap), torch.float32), ((G, cap), torch.float32),
                    ((G, cap) if own_logs else (1,), torch.int32), ((G, cap) if own_logs else (1,), torch.int32))
    bucket_sum, bucket_cnt = (zf[0][0], zf[0][1]) if bucket_idx is not None else (None, None)    # (written by the finalize kernel)
    loss, lse = zf[1], zf[2]
    n_valid, rank = (zf[3], zf[4]) if own_logs else (None, None)
    s_pos = torch.empty(G, cap, dtype=torch.float32, device=dev)
    c = types.SimpleNamespace(q_idx=q_idx, p_idx=p_idx, n_tok_dev=n_tok_dev, tok_cap=tok_cap, cap=cap, groups=G, dim=D, n_neg=n_neg,
                              thres=float(thres), negs=negs, lse=lse, s_pos=s_pos, bucket_idx=bucket_idx, n_buckets=int(n_buckets),
                              bucket_sum=bucket_sum, bucket_cnt=bucket_cnt)
    if path == "wide":
        from . import wide
        return wide.nce_fwd_wide(c, q_rows, p_rows, logit_scale, want_logs, float(ihn_beta), loss, n_valid, rank)
    if path == "shared":
        cls, own, ssum, n_valid, rank = _nce_fwd_shared(c, q_rows, p_rows, logit_scale, want_logs, log_group, p_row_mask, window, prep)
    else:
        cls, own, ssum, n_valid, rank = _nce_fwd_tokens(c, q_rows, p_rows, logit_scale, log_group, p_row_mask, n_valid, rank)
    lib.call("mhr_nce_finalize", ssum.data_ptr(), s_pos.data_ptr(), G, n_tok_dev.data_ptr(), cap,
             logit_scale.data_ptr(), loss.data_ptr(), lse.data_ptr(), _ptr(n_valid), _ptr(bucket_idx), int(n_buckets),
             _ptr(bucket_sum), _ptr(bucket_cnt), _stream())
    return cls(loss, n_valid, rank, **vars(c), **own)


def nce_bwd(sv, w, logit_scale, q_idx, p_idx, dq_rows, dp_rows, d_negs=None, d_logit_scale=None, want_negs=True, lw_row=None,
            exclusive_q_rows=False, dq_rows_zero=False):
    """w [G, tok_cap] f32 = dLoss/dloss[g, t] - or [G, n_buckets] when the forward was given bucket_idx (every token
    of a bucket then has the same weight).  Accumulates into dq_rows [Rq, D] / dp_rows [Rp, D] (f32, the
    forward's shared row spaces); returns (d_negs [G, n_neg, D] f32, d_logit_scale [1]).  q_idx / p_idx are the
    forward's index lists (the padded copies saved by nce_fwd are what the kernels read).  want_negs=False skips the
    negative-side product (frozen negatives, e.g. the HLLM twin's cached item tower) and returns d_negs = None.
    exclusive_q_rows: no two (group, query-row) pairs of the forward name the same row of dq_rows (the groups read disjoint
    decoding heads): the row-wise backward then adds with plain read-modify-writes instead of float atomics.
    dq_rows_zero (with exclusive_q_rows): dq_rows holds zeros and nothing but this call writes it before it is read: the row-wise
    backward stores the row gradients without reading the zeros back (same bits)."""
    dev = sv.negs.device
    D, cap, G = sv.dim, sv.cap, sv.groups
    if w.dim() == 1:
        w = w[None]
    bucketed = sv.bucket_idx is not None and w.shape == (G, sv.n_buckets) and sv.n_buckets != sv.tok_cap
    if d_negs is None and want_negs:
        d_negs = torch.zeros(G, sv.n_neg, D, dtype=torch.float32, device=dev)
    if d_logit_scale is None:
        d_logit_scale = torch.zeros(1, dtype=torch.float32, device=dev)
    if cap != sv.tok_cap and not bucketed:
        w = torch.nn.functional.pad(w, (0, cap - sv.tok_cap))
    w = w.contiguous()
    _chk(w, "w", torch.float32)
    _chk(dq_rows, "dq_rows", torch.float32)
    _chk(dp_rows, "dp_rows", torch.float32)
    wb_ptr, nb = (sv.bucket_idx.data_ptr(), sv.n_buckets) if bucketed else (0, 0)      # per-bucket weights: the kernels look them up
    if sv.wide:
        from . import wide
        w_tok = torch.gather(w, 1, sv.bucket_idx.long().clamp(0, sv.n_buckets - 1)) if bucketed else w
        wide.nce_bwd_wide(sv, w_tok, logit_scale, dq_rows, dp_rows, d_negs, d_logit_scale)
    elif sv.shared:
        _nce_bwd_shared(sv, w, wb_ptr, nb, logit_scale, dq_rows, dp_rows, d_negs, d_logit_scale, want_negs, lw_row,
                        (2 if dq_rows_zero else 1) if exclusive_q_rows else 0)
    else:
        _nce_bwd_tokens(sv, w, wb_ptr, nb, logit_scale, dq_rows, dp_rows, d_negs, d_logit_scale, want_negs)
    return d_negs, d_logit_scale


def _nce_bwd_shared(sv, w, wb_ptr, nb, logit_scale, dq_rows, dp_rows, d_negs, d_logit_scale, want_negs, lw_row, exclusive_rows):
    """Row-wise / target-wise kernels for window-structured lists, else per-token atomics; then the negative-side product over the rows.
    exclusive_rows: mhr_nce_shared_bwd_rows' mode (0 float atomics, 1 read-modify-write, 2 store into zeroed rows)."""
    dev, D, cap, G, st = sv.negs.device, sv.dim, sv.cap, sv.groups, _stream()
    dn_ptr = d_negs.data_ptr() if want_negs else 0
    if lw_row is None:                   # (+inf: a row the kernels do not visit contributes nothing to the negative-side product)
        lw_row = torch.full((G, sv.row_cap), float("inf"), dtype=torch.float32, device=dev)
    assert lw_row.shape == (G, sv.row_cap)
    dn_fix = dls_part = None
    if DETERMINISTIC and sv.window is not None:
        dn_fix = torch.zeros(d_negs.shape, dtype=torch.int64, device=dev) if want_negs else None
        dls_part = torch.zeros(G * 1024, dtype=torch.float32, device=dev)
    if sv.window is not None:            # window-structured lists: sums formed where they land, no per-token atomics
        tos, L_, P_ = sv.window
        _timed_call("mhr_nce_shared_bwd_rows", sv.qn.data_ptr(), sv.u.data_ptr(), sv.q_inv.data_ptr(), sv.row_q.data_ptr(),
                    sv.row_first.data_ptr(), sv.n_row_dev.data_ptr(), sv.row_cap, sv.pn.data_ptr(), D, G, cap,
                    logit_scale.data_ptr(), sv.lse.data_ptr(), w.data_ptr(), sv.s_pos.data_ptr(), sv.p_idx.data_ptr(),
                    dq_rows.data_ptr(), d_logit_scale.data_ptr(), lw_row.data_ptr(), wb_ptr, nb, sv.negs.data_ptr(), sv.n_neg,
                    sv.fix_words.data_ptr(), sv.n_p_rows, _ptr(sv.fix_slot), sv.fix_any.data_ptr(), dn_ptr,
                    int(exclusive_rows), _ptr(dn_fix), _ptr(dls_part), st)
        if dls_part is not None:         # the workgroups' partials of d(logit_scale), folded in index order
            lib.call("mhr_det_sum_into", dls_part.data_ptr(), dls_part.numel(), logit_scale.data_ptr(), 1, d_logit_scale.data_ptr(), st)
        _timed_call("mhr_nce_shared_bwd_targets", sv.qn.data_ptr(), sv.row_cap, sv.tok2row.data_ptr(), tos.data_ptr(),
                    sv.n_tok_dev.data_ptr(), G, tos.shape[1], cap, int(L_), int(P_), sv.pn.data_ptr(), sv.p_inv.data_ptr(), D,
                    logit_scale.data_ptr(), sv.lse.data_ptr(), w.data_ptr(), sv.s_pos.data_ptr(), wb_ptr, nb, sv.n_p_rows,
                    dp_rows.data_ptr(), st)
    else:
        lw_tok = torch.empty(G, cap, dtype=torch.float32, device=dev)
        _timed_call("mhr_nce_shared_bwd_tokens", sv.qn.data_ptr(), sv.u.data_ptr(), sv.q_inv.data_ptr(), sv.row_cap,
                    sv.tok2row.data_ptr(), sv.pn.data_ptr(), D, G, sv.n_tok_dev.data_ptr(), cap, logit_scale.data_ptr(),
                    sv.lse.data_ptr(), w.data_ptr(), sv.p_inv.data_ptr(), sv.s_pos.data_ptr(), sv.q_idx.data_ptr(),
                    sv.p_idx.data_ptr(), dq_rows.data_ptr(), dp_rows.data_ptr(), d_logit_scale.data_ptr(), lw_tok.data_ptr(),
                    wb_ptr, nb, sv.negs.data_ptr(), sv.n_neg, sv.fix_words.data_ptr(), sv.n_p_rows, _ptr(sv.fix_slot),
                    sv.fix_any.data_ptr(), dn_ptr, st)
        if want_negs:
            lib.call("mhr_nce_row_lw", lw_tok.data_ptr(), sv.row_first.data_ptr(), sv.n_row_dev.data_ptr(), G, cap, sv.row_cap,
                     lw_row.data_ptr(), st)
    if want_negs:
        _timed_call("mhr_nce_bwd_negs", sv.qn.data_ptr(), sv.negs.data_ptr(), _ptr(sv.supp), sv.n_neg, D, G,
                    sv.n_row_dev.data_ptr(), sv.row_cap, logit_scale.data_ptr(), lw_row.data_ptr(), d_negs.data_ptr(),
                    _ptr(dn_fix), st)
        if dn_fix is not None:           # fixed-point accumulators (tiles + suppressed-pair corrections) -> d_negs
            lib.call("mhr_det_flush", dn_fix.data_ptr(), d_negs.data_ptr(), d_negs.numel(), st)


def _nce_bwd_tokens(sv, w, wb_ptr, nb, logit_scale, dq_rows, dp_rows, d_negs, d_logit_scale, want_negs):
    """Per-token backward: the token kernel (dq, dp, d(logit_scale), the row weights), then the negative-side product."""
    dev, D, cap, G, st = sv.negs.device, sv.dim, sv.cap, sv.groups, _stream()
    lw = torch.empty(G, cap, dtype=torch.float32, device=dev)     # lse log2e - log2 w: written by bwd_tokens, read by bwd_negs
    dq_fix = dp_fix = dls_part = dn_fix = None
    if DETERMINISTIC:             # order-independent accumulation (include/mhr.h: deterministic mode)
        dq_fix = torch.zeros(dq_rows.shape, dtype=torch.int64, device=dev)
        dp_fix = torch.zeros(dp_rows.shape, dtype=torch.int64, device=dev)
        dls_part = torch.zeros(G * 2048 * 4, dtype=torch.float32, device=dev)
        dn_fix = torch.zeros(d_negs.shape, dtype=torch.int64, device=dev) if want_negs else None
    _timed_call("mhr_nce_bwd_tokens", sv.qn.data_ptr(), sv.pn.data_ptr(), sv.u.data_ptr(), D,
                G, sv.n_tok_dev.data_ptr(), cap, logit_scale.data_ptr(), sv.lse.data_ptr(), w.data_ptr(), sv.q_inv.data_ptr(),
                sv.p_inv.data_ptr(), sv.s_pos.data_ptr(), sv.q_idx.data_ptr(), sv.p_idx.data_ptr(), dq_rows.data_ptr(),
                dp_rows.data_ptr(), d_logit_scale.data_ptr(), lw.data_ptr(), wb_ptr, nb, _ptr(dq_fix), _ptr(dp_fix),
                _ptr(dls_part), st)
    if dq_fix is not None:
        lib.call("mhr_det_flush", dq_fix.data_ptr(), dq_rows.data_ptr(), dq_rows.numel(), st)
        lib.call("mhr_det_flush", dp_fix.data_ptr(), dp_rows.data_ptr(), dp_rows.numel(), st)
        lib.call("mhr_det_sum_into", dls_part.data_ptr(), dls_part.numel(), logit_scale.data_ptr(), 1, d_logit_scale.data_ptr(), st)
    if want_negs:
        _timed_call("mhr_nce_bwd_negs", sv.qn.data_ptr(), sv.negs.data_ptr(), sv.supp.data_ptr(), sv.n_neg, D, G,
                    sv.n_tok_dev.data_ptr(), cap, logit_scale.data_ptr(), lw.data_ptr(), d_negs.data_ptr(), _ptr(dn_fix), st)
        if dn_fix is not None:
            lib.call("mhr_det_flush", dn_fix.data_ptr(), d_negs.data_ptr(), d_negs.numel(), st)


# ------------------------------------------------------------------------------------------------
# catalog scoring / top-k / merge
# ------------------------------------------------------------------------------------------------
def catalog_emit(users, H, items, tag_bits, row_bits, tau, hist_ptr, hist_items, cap, item_begin=0, item_stride=1,
                 cand=None, n_items=None):
    n_rows, D = users.shape
    dev = users.device
    if cand is None:
        cand = (torch.empty(n_rows, cap, dtype=torch.float32, device=dev),
                torch.empty(n_rows, cap, dtype=torch.int32, device=dev),
                torch.zeros(n_rows, dtype=torch.int32, device=dev))
    else:
        cand[2].zero_()
    _timed_call("mhr_catalog_score_emit", users.data_ptr(), n_rows, H, items.data_ptr(),
                items.shape[0] if n_items is None else n_items, D, item_begin,
             item_stride, _ptr(tag_bits), row_bits.data_ptr(), tau.data_ptr(), _ptr(hist_ptr), _ptr(hist_items),
             cand[0].data_ptr(), cand[1].data_ptr(), cand[2].data_ptr(), cap, _stream())
    return cand


def topk_select(cand, cap, k):
    val, idx, cnt = cand
    n_rows = cnt.shape[0]
    dev = cnt.device
    out_val = torch.empty(n_rows, k, dtype=torch.float32, device=dev)
    out_idx = torch.empty(n_rows, k, dtype=torch.int64, device=dev)
    kth = torch.empty(n_rows, dtype=torch.float32, device=dev)
    status = torch.empty(n_rows, dtype=torch.int32, device=dev)
    _timed_call("mhr_topk_select", val.data_ptr(), idx.data_ptr(), cnt.data_ptr(), cap, n_rows, k, out_val.data_ptr(),
             out_idx.data_ptr(), kth.data_ptr(), status.data_ptr(), _stream())
    return out_val, out_idx, kth, status


def _slices_for(n_rows, n_tiles):
    """item slices of the sliced emit: about 512 workgroups (2 per CU), a multiple of 8 (one per XCD), <= n_tiles - decided by
    the library (mhr_catalog_emit_slices; its workspace query sizes the candidate lists)."""
    return int(lib.load().mhr_catalog_emit_slices(int(n_rows), int(n_tiles) * 32))


def catalog_emit_sliced(users, items, n_items, tag_bits, row_bits, tau, cap_s, item_begin=0, item_stride=1):
    """-> (cand_val, cand_idx [n_rows, n_lists, cap_s], cand_cnt [n_rows, n_lists], n_lists = 2 x item slices).
    No history filter (topk_select_sliced applies it)."""
    n_rows, D = users.shape
    dev = users.device
    n_sel = (n_items - item_begin + item_stride - 1) // item_stride
    n_slices = _slices_for(n_rows, (n_sel + 31) // 32)
    val = torch.empty(n_rows, 2 * n_slices, cap_s, dtype=torch.float32, device=dev)      # 2 lists per slice (one per wave half)
    idx = torch.empty(n_rows, 2 * n_slices, cap_s, dtype=torch.int32, device=dev)
    cnt = torch.empty(n_rows, 2 * n_slices, dtype=torch.int32, device=dev)
    _timed_call("mhr_catalog_score_emit_sliced", users.data_ptr(), n_rows, items.data_ptr(), n_items, items.shape[0], D,
                item_begin, item_stride, _ptr(tag_bits), row_bits.data_ptr(), tau.data_ptr(), val.data_ptr(), idx.data_ptr(),
                cnt.data_ptr(), n_slices, cap_s, _stream())
    return val, idx, cnt, 2 * n_slices


def pack_tiles(x, n_sel=None, row_begin=0, row_stride=1, tiles_per_block=8):
    """Rows {row_begin + j row_stride} of x [n, D] bf16 -> the wide scorer's packed tile images (uint8 tensor)."""
    _chk(x, "x", torch.bfloat16)
    n, D = x.shape
    if n_sel is None:
        n_sel = (n - row_begin + row_stride - 1) // row_stride
    nbytes = lib.load().mhr_pack_tiles_bytes(n_sel, D, tiles_per_block)
    out = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    lib.call("mhr_pack_tiles", x.data_ptr(), n, D, row_begin, row_stride, n_sel, tiles_per_block, out.data_ptr(), _stream())
    return out


def pack_tiles_t(x, n_sel=None, tiles_per_block=8):
    """Columns [0, n_sel) of x [n_k, ld] bf16 as packed rows (the contraction index runs down x's rows): the transposed operand
    of mhr_wide_gemm_nt.  -> (uint8 tensor, padded contraction length)."""
    _chk(x, "x", torch.bfloat16)
    n_k, ld = x.shape
    n_sel = ld if n_sel is None else int(n_sel)
    k_pad = -(-n_k // 64) * 64
    out = torch.empty(lib.load().mhr_pack_tiles_bytes(n_sel, k_pad, tiles_per_block), dtype=torch.uint8, device=x.device)
    lib.call("mhr_pack_tiles_t", x.data_ptr(), n_k, ld, n_sel, tiles_per_block, out.data_ptr(), _stream())
    return out, k_pad


def catalog_emit_wide(users_p, n_rows, D, items_p, n_items, tag_bits, row_bits, tau, cap_s, item_begin=0, item_stride=1):
    """Feature dims beyond 256 (a multiple of 64): the LDS-tiled MFMA scorer with the fused threshold emit
    (csrc/catalog_wide.hip) on PACKED operands (pack_tiles: users with 4 tiles per block, the selected items with 8).
    -> (cand_val, cand_idx [n_rows, n_lists, cap_s], cand_cnt [n_rows, n_lists], n_lists = 4 x slices)."""
    dev = users_p.device
    n_slices = lib.load().mhr_catalog_wide_slices(n_rows)        # fixed by the kernel's XCD layout (32 ... 256)
    val = torch.empty(n_rows, 4 * n_slices, cap_s, dtype=torch.float32, device=dev)
    idx = torch.empty(n_rows, 4 * n_slices, cap_s, dtype=torch.int32, device=dev)
    cnt = torch.empty(n_rows, 4 * n_slices, dtype=torch.int32, device=dev)
    _timed_call("mhr_catalog_score_emit_wide", users_p.data_ptr(), n_rows, items_p.data_ptr(), n_items, D, item_begin, item_stride,
                _ptr(tag_bits), row_bits.data_ptr(), tau.data_ptr(), val.data_ptr(), idx.data_ptr(), cnt.data_ptr(), n_slices,
                cap_s, _stream())
    return val, idx, cnt, 4 * n_slices


def topk_select_sliced(cand, H, hist_ptr, hist_items, k):
    """-> (values [n_rows,k], indices [n_rows,k], kth value, valid-candidate count, overflow status)."""
    val, idx, cnt, n_slices = cand
    n_rows, _, cap_s = val.shape
    dev = val.device
    out_val = torch.empty(n_rows, k, dtype=torch.float32, device=dev)
    out_idx = torch.empty(n_rows, k, dtype=torch.int64, device=dev)
    kth = torch.empty(n_rows, dtype=torch.float32, device=dev)
    count = torch.empty(n_rows, dtype=torch.int32, device=dev)
    status = torch.empty(n_rows, dtype=torch.int32, device=dev)
    _timed_call("mhr_topk_select_sliced", val.data_ptr(), idx.data_ptr(), cnt.data_ptr(), n_slices, cap_s, n_rows, H,
                _ptr(hist_ptr), _ptr(hist_items), k, out_val.data_ptr(), out_idx.data_ptr(), kth.data_ptr(), count.data_ptr(),
                status.data_ptr(), _stream())
    return out_val, out_idx, kth, count, status


def sub_history(hist_ptr, hist_items, users_f):
    """CSR history (ptr [B+1] int32, items sorted per user) restricted to the users `users_f` [F] (ascending)."""
    if hist_ptr is None:
        return None, None
    dev = hist_ptr.device
    lens = (hist_ptr[1:] - hist_ptr[:-1])[users_f].long()
    sub_ptr = torch.zeros(users_f.numel() + 1, dtype=torch.int32, device=dev)
    sub_ptr[1:] = torch.cumsum(lens, 0).int()
    starts = hist_ptr[:-1][users_f].long()
    off = torch.arange(int(lens.sum()), device=dev) - torch.repeat_interleave(sub_ptr[:-1].long(), lens)
    return sub_ptr, hist_items[torch.repeat_interleave(starts, lens) + off].contiguous()


TopkPlan = collections.namedtuple("TopkPlan", "k k_min target s1 s2 t1 t2")
TopkResult = collections.namedtuple("TopkResult", "values indices tau flagged")       # tau None: the scorer reports no threshold
# The scorer of one call (decode_path names it; built by stream_scorer, wide.mfma_scorer or wide.gemm_scorer), as topk_decode uses it:
# all_candidates() -> (values, indices) where the catalog is small enough to keep every score, else None; candidates() -> (tau
# [rows], candidate lists above it in topk_select_sliced's form); exact_rows(rows, sub_ptr, sub_items) -> (values, indices), the
# path's own repair of the rows `rows`; k_flag: the candidates a row needs; reports_tau: whether its tau certifies anything
Scorer = collections.namedtuple("Scorer", "all_candidates candidates exact_rows k_flag reports_tau")


def topk_plan(N, k, k_min=None, target=None):
    """The threshold budget of one decode, plain ints: a row needs k_min (<= k) candidates, `target` are aimed at; sample pass i
    scores every s_i-th item and hands on its t_i-th largest score."""
    k_min = k if k_min is None else min(k, k_min)
    if target is None:
        # candidates aimed at per row.  The threshold is the (target/s2)-th largest of a 1/s2 sample: its rank estimate
        # scatters by about 1/sqrt(target/s2), so 2.5 k leaves > 5 sigma before a row would come up short (and such a
        # row is only re-run, never wrong); every candidate above what is needed costs a divergent slow-path visit.
        target = max(512, int(2.5 * k_min))
    s1 = max(1, -(-N // 2048))
    # second sample: dense enough that the threshold is the ~50th largest of the sample (its rank estimate then scatters by
    # ~14 %: a row comes up short of k candidates at > 4 sigma; at N = 2^20 a 1 / 32 sample left 2.4 sigma and flagged rows -
    # each an exact re-run - in most batches)
    s2 = max(1, min(-(-N // 32768), target // 48))
    t1 = min(1024, max(8, -(-3 * target // s1)))           # first threshold: about 3x looser than the rank aimed at (a tighter one
                                                           # starves the second sample and, as the fallback threshold, the candidates)
    t2 = min(1024, max(k_min // s2 + 1, target // s2))     # (the select kernel picks at most 1024)
    return TopkPlan(k, k_min, target, s1, s2, t1, t2)


def decode_path(D, users_dtype, items_dtype):
    """The scorer of a catalog decode: "stream" (register-stationary, csrc/catalog.hip) at its feature dims; "mfma" (LDS-tiled,
    csrc/catalog_wide.hip) for bf16 operands at any other multiple of 64; else "gemm" (library GEMM + csrc/wide.hip)."""
    if D in STREAM_DIMS:
        return "stream"
    return "mfma" if D % 64 == 0 and users_dtype == items_dtype == torch.bfloat16 else "gemm"


def _ninf(rows):
    return torch.full((rows.shape[0],), float("-inf"), dtype=torch.float32, device=rows.device)


def sampled_tau(emit, cap1, cap2, plan, H, hist_ptr, hist_items):
    """Threshold of the stream and the MFMA scorer: two strided sample passes through the scorer's own emit(tau, cap_s, sample)
    (sample 0: every item, 1 / 2: every s1-th / s2-th), list capacities cap1 / cap2 -> (tau, pass 2's sorted values, st1, st2)."""
    # pass 1: every s1-th item, all scores (<= 2048 per row) -> the t1-th largest bounds the top ~0.4 %
    _, _, kth1, _, st1 = topk_select_sliced(emit(None, cap1, 1), H, hist_ptr, hist_items, plan.t1)
    # pass 2: every s2-th item above kth1 -> the t2-th largest estimates the score of rank ~target
    ov2, _, kth2, _, st2 = topk_select_sliced(emit(kth1, cap2, 2), H, hist_ptr, hist_items, plan.t2)
    tau = torch.empty_like(kth1)
    lib.call("mhr_topk_pick_tau", kth1.data_ptr(), kth2.data_ptr(), st1.data_ptr(), st2.data_ptr(), tau.shape[0], tau.data_ptr(), _stream())
    return tau, ov2, st1, st2


def stream_scorer(users, H, items, N, tag_bits, row_bits, hist_ptr, hist_items, plan, cap):
    """Feature dims of STREAM_DIMS: the sliced emit; catalogs of at most `cap` items and the repair go through the atomic-list
    emit with tau = -inf (every admissible score kept) + the whole-row select."""
    n_rows = users.shape[0]
    def emit(tau, cap_s, sample=0):
        return catalog_emit_sliced(users, items, N, tag_bits, row_bits, _ninf(users) if tau is None else tau, cap_s, 0,
                                   (1, plan.s1, plan.s2)[sample])

    def every_score(rows, ptr, hist):
        u, bits = (users, row_bits) if rows is None else (users[rows].contiguous(), row_bits[rows].contiguous())
        return topk_select(catalog_emit(u, H, items, tag_bits, bits, _ninf(u), ptr, hist, N, n_items=N), N, plan.k)[:2]

    def candidates():
        nt1 = -(-(-(-N // plan.s1)) // 32)                                 # tiles of the first sample
        tau = sampled_tau(emit, 32 * -(-nt1 // _slices_for(n_rows, nt1)), 32, plan, H, hist_ptr, hist_items)[0]
        return tau, emit(tau, max(32, 4 * -(-plan.target // _slices_for(n_rows, -(-N // 32))) + 16))

    return Scorer(lambda: every_score(None, hist_ptr, hist_items) if N <= cap else None, candidates, every_score, plan.k_min, True)


def topk_decode(sc, H, row_bits, hist_ptr, hist_items, k, stats=None, defer_check=None):
    """The decode scheme, once, for whichever Scorer it is handed: a small catalog keeps every score; otherwise per-row thresholds,
    one full pass into candidate lists, the exact select, a flag on every row that cannot be trusted (list overflow, fewer than
    k_flag candidates) and - after the call's one host read - the exact re-run of the flagged users' rows.  -> TopkResult."""
    n_rows, dev = row_bits.shape[0], row_bits.device
    small = sc.all_candidates()
    if small is not None:
        return TopkResult(*small, _ninf(row_bits) if sc.reports_tau else None, None)
    tau, cand = sc.candidates()
    ov, oi, _, cnt, st = topk_select_sliced(cand, H, hist_ptr, hist_items, k)
    flagged = torch.empty(n_rows, dtype=torch.bool, device=dev)
    any_flag = defer_check if defer_check is not None else torch.empty(1, dtype=torch.int32, device=dev)
    lib.call("mhr_topk_flag", st.data_ptr(), cnt.data_ptr(), row_bits.data_ptr(), tau.data_ptr(), int(sc.k_flag), n_rows,
             flagged.data_ptr(), any_flag.data_ptr(), _stream())
    if stats is not None:
        stats["mean_candidates"] = float(cnt.float().mean())
        stats["flagged_rows"] = int(flagged.sum())
    if defer_check is None and bool(any_flag.item()):     # one host sync per batch (defer_check: the caller's, with its own flags)
        users_f = torch.nonzero(flagged.view(-1, H).any(dim=1)).flatten()
        rows_f = (users_f[:, None] * H + torch.arange(H, device=dev)[None, :]).flatten()
        ov[rows_f], oi[rows_f] = sc.exact_rows(rows_f, *sub_history(hist_ptr, hist_items, users_f))
        tau = tau.index_fill(0, rows_f, float("-inf"))
    return TopkResult(ov, oi, tau if sc.reports_tau else None, flagged)


def catalog_decode(users, H, items, tag_bits, row_bits, hist_ptr, hist_items, k, cap=4096, target=None, stats=None, n_items=None,
                   k_min=None, margin=None, defer_check=None, chunk=None):
    """Exact per-row top-k over the whole catalog (value desc, index asc), rows = (user, head) pairs: the scorer decode_path names,
    budgeted by topk_plan, under topk_decode -> TopkResult (values [B*H,k] f32, indices [B*H,k] i64, tau [B*H] f32: the emit
    threshold each row's candidates were collected with; -inf: every admissible item was a candidate).
    users [B*H, D] bf16 normalised, items [>= N, D] bf16 normalised (rows beyond n_items = N are padding: give the
    table round_up(N, 32) rows and the item tiles stream unclamped).  cap / chunk: the stream / GEMM scorer's own sizes.
    k_min (default k): rows with fewer than k_min candidates are re-run exactly; with k_min < k a row may return fewer than
    k finite entries (its list then holds EVERY item scoring >= its threshold).
    margin: the caller re-ranks everything within `margin` of the k_min-th score; only the MFMA scorer's threshold needs it.
    defer_check (int32 device tensor [>= 1]; the stream scorer only): write "some row failed" into defer_check[0] and return,
    instead of reading it here (a host sync) and repairing; the caller reads it with its own flags and comes back (catalog_topk_exact)."""
    from . import wide
    N = items.shape[0] if n_items is None else int(n_items)
    path, operands = decode_path(users.shape[1], users.dtype, items.dtype), (users, H, items, N, tag_bits, row_bits, hist_ptr, hist_items)
    if path == "stream":
        sc = stream_scorer(*operands, topk_plan(N, k, k_min, target), cap)
    elif path == "mfma":
        sc = wide.mfma_scorer(*operands, topk_plan(N, k, k_min, target), margin)
    else:
        sc = wide.gemm_scorer(*operands, k, target, chunk or wide.ITEM_CHUNK)
    return topk_decode(sc, H, row_bits, hist_ptr, hist_items, k, stats, defer_check if path == "stream" else None)


def catalog_topk(users, H, items, tag_bits, row_bits, hist_ptr, hist_items, k, cap=4096, target=None, stats=None, n_items=None,
                 k_min=None, margin=None, defer_check=None):
    """catalog_decode -> (values, indices)."""
    return catalog_decode(users, H, items, tag_bits, row_bits, hist_ptr, hist_items, k, cap, target, stats, n_items, k_min, margin,
                          defer_check)[:2]


DENSE_ROWS_CHUNK = 128     # rows scored densely per launch (128 x 454 k x 8 B = 465 MB of scratch at cfg1)


def dense_rows_topk(users, H, items, n_items, tag_bits, row_bits, hist_ptr, hist_items, rows, k):
    """Exact top-k (value desc, index asc) of the rows `rows` (int32 [F], indices into users [B*H, D]) with EVERY score
    kept: `mhr_catalog_score_rows_dense` (fp32 accumulation of fp32 or bf16 operands, tag / pad / history masks in place)
    + the exact select over the whole row.  hist_ptr / hist_items: the CSR history of ALL users (row // H picks the user).
    The rare path of the decode (rows the threshold scorers cannot certify); reference hstu.py:965-1015, trainer.py:724-726,
    collector.py:245.  -> (values [F, k] f32, indices [F, k] i64)."""
    N = int(n_items)
    dev = users.device
    if users.dtype != items.dtype or users.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"dense_rows_topk: users / items must both be fp32 or both bf16 (got {users.dtype}, {items.dtype})")
    if not (users.is_cuda and users.is_contiguous() and items.is_contiguous()):
        raise ValueError("dense_rows_topk: contiguous GPU tensors only (no CPU path)")
    dt = lib.F32 if users.dtype == torch.float32 else lib.BF16
    rows = rows.to(torch.int32).contiguous()
    F_ = rows.numel()
    ov = torch.empty(F_, k, dtype=torch.float32, device=dev)
    oi = torch.empty(F_, k, dtype=torch.int64, device=dev)
    for r0 in range(0, F_, DENSE_ROWS_CHUNK):
        r1 = min(F_, r0 + DENSE_ROWS_CHUNK)
        val = torch.empty(r1 - r0, N, dtype=torch.float32, device=dev)
        idx = torch.empty(r1 - r0, N, dtype=torch.int32, device=dev)
        cnt = torch.empty(r1 - r0, dtype=torch.int32, device=dev)
        _timed_call("mhr_catalog_score_rows_dense", users.data_ptr(), items.data_ptr(), dt, users.shape[1], N, rows[r0:r1].data_ptr(),
                    r1 - r0, H, _ptr(tag_bits), row_bits.data_ptr(), _ptr(hist_ptr), _ptr(hist_items), val.data_ptr(),
                    idx.data_ptr(), cnt.data_ptr(), _stream())
        fv, fi, _, _ = topk_select((val, idx, cnt), N, k)
        ov[r0:r1], oi[r0:r1] = fv, fi
    return ov, oi


BF16_SCORE_ERR = 2.0 ** -8       # |u_bf16 . i_bf16 - u . i| for unit vectors u, i (each component rounded to 8 bits)


def _margin_slots(N, k, D):
    """Candidates kept per row by the exact decodes: the margin set must fit.  Wide feature dims concentrate the cosines of
    (near-)random embeddings around 0 (std 1 / sqrt(D)), so a 2^-7 margin below the k-th score holds several hundred items there:
    keep the maximum."""
    k2 = min(N - 1, 1024, max(2 * k + 64, k + 256) if D <= 256 else 1024)
    return k if k2 <= k else k2


def _exact_attempt(users_bf, H, items_bf, N, tag_bits, row_bits, hist_ptr, hist_items, k, k2, flags, defer, stats, target, rescore):
    """One pass of the exact decodes (catalog_topk_exact, catalog_topk_mean): the bf16 scorer's candidate lists (everything above a
    per-row threshold tau near the rank-2.5k score), the best k2 of them sorted, the margin set of every row re-scored by
    `rescore(cand_idx [n_rows,k2] i64, cand_cnt [n_rows] i32, out_val [n_rows,k2] f32, out_idx [n_rows,k2] i32)` in fp32, the exact
    select on the re-scored values.  A row is CERTIFIED when its margin [kth - 2^-7, ...) lies above tau (nothing that could enter
    the fp32 top-k was left below the threshold) and does not fill all k2 slots.  flags (int32 [>= 2], device): [0] the bf16 pass's
    "some row failed" when `defer` (else it is read and repaired inside catalog_decode), [1] "some row is uncertified".
    -> (values [n_rows,k], indices [n_rows,k], margin counts, uncertified [n_rows] bool)."""
    n_rows, dev = users_bf.shape[0], users_bf.device
    kk = min(k, k2)
    bv, bi, tau, _ = catalog_decode(users_bf, H, items_bf, tag_bits, row_bits, hist_ptr, hist_items, k2, stats=stats, n_items=N,
                                    k_min=k, margin=2 * BF16_SCORE_ERR, defer_check=flags[0:1] if defer else None, target=target)
    if tau is None:
        # the GEMM scorer (its small-catalog form too) reports no threshold, which certifies nothing: +inf flags every row and
        # all of them take the dense fp32 repair (the other scorers' small-catalog forms report tau = -inf)
        tau = torch.full((n_rows,), float("inf"), dtype=torch.float32, device=dev)
    bv = bv.contiguous()
    cnt = torch.empty(n_rows, dtype=torch.int32, device=dev)          # the margin set: a prefix of the sorted list
    lib.call("mhr_topk_margin_count", bv.data_ptr(), n_rows, k2, kk, 2 * BF16_SCORE_ERR, cnt.data_ptr(), _stream())
    rv = torch.empty(n_rows, k2, dtype=torch.float32, device=dev)
    ri = torch.empty(n_rows, k2, dtype=torch.int32, device=dev)
    rescore(bi, cnt, rv, ri)
    ov, oi, _, st = topk_select((rv, ri, cnt), k2, k)
    # uncertified rows: the margin reaches below the emit threshold, or fills the candidate list (the (k2+1)-th bf16 score
    # might be inside it too)
    full = torch.empty(n_rows, dtype=torch.bool, device=dev)
    lib.call("mhr_topk_uncertified", cnt.data_ptr(), bv.data_ptr(), k2, kk, tau.contiguous().data_ptr(), 1 if k2 < N - 1 else 0,
             2 * BF16_SCORE_ERR, n_rows, full.data_ptr(), flags[1:2].data_ptr(), _stream())
    return ov, oi, cnt, full


def catalog_topk_exact(users_f32, H, items_bf, items_f32, tag_bits, row_bits, hist_ptr, hist_items, k, n_items=None, stats=None,
                       target=None, defer=False):
    """Per-row top-k ranked on FP32 scores of fp32 operands - the reference's score path (hstu.py:965-979: fp32 normalise,
    fp32 matmul; collector.py:245 torch.topk) - without a [B, H, N] tensor.  The bf16 scorer finds every candidate whose bf16
    score lies within 2^-7 of the k-th bf16 score (a superset of the fp32 top-k: the two scores differ by at most 2^-8),
    `mhr_rescore_f32` re-scores those few hundred candidates per row from the fp32 rows, and the exact select picks k by
    (fp32 value desc, index asc).  Rows whose margin set cannot be certified (more than 1024 near-ties) fall back to dense
    fp32 scoring of that row.  users_f32 [B*H, D] fp32 normalised; items_bf [>= N, D] bf16 / items_f32 [N, D] fp32 normalised.
    target: the bf16 pass's candidate budget per row (catalog_topk; tests shrink it to force its repair path).
    defer=True: enqueue everything WITHOUT the host read and return (values, indices, finish): finish() reads the two flags, repairs
    the rare rows in place and returns the final (values, indices) - the split the replayed evaluation step needs (everything in
    front of finish() is capturable: REC/trainer/trainer.py:_EvalGraph)."""
    n_rows, D = users_f32.shape
    N = items_f32.shape[0] if n_items is None else int(n_items)
    dev = users_f32.device
    users_bf = users_f32.to(torch.bfloat16).contiguous()
    k2 = _margin_slots(N, k, D)
    # ONE host read per call: the bf16 pass leaves its "some row failed" flag on the device (defer_check) next to this function's
    # "some row is uncertified" flag; only when the first is set - thresholds that came up short, never seen on trained or random
    # embeddings - the pass is repeated with its own check-and-repair
    deferred = decode_path(D, users_bf.dtype, items_bf.dtype) == "stream" and N > 4096 and stats is None
    flags = torch.empty(2, dtype=torch.int32, device=dev)
    _chk(users_f32, "users_f32", torch.float32)
    _chk(items_f32, "items_f32", torch.float32)

    def rescore(bi, cnt, rv, ri):
        lib.call("mhr_rescore_f32", users_f32.data_ptr(), items_f32.data_ptr(), D, N, bi.data_ptr(), n_rows, k2, cnt.data_ptr(),
                 rv.data_ptr(), ri.data_ptr(), _stream())

    def attempt(defer):
        return _exact_attempt(users_bf, H, items_bf, N, tag_bits, row_bits, hist_ptr, hist_items, k, k2, flags, defer, stats, target,
                              rescore)

    if defer and not deferred:
        raise ValueError("catalog_topk_exact(defer=True) needs the streaming scorer's deferred check (feature dim <= 256, N > 4096, no stats)")
    ov, oi, cnt, full = attempt(deferred)

    def finish():
        nonlocal ov, oi, cnt, full
        got = flags.tolist()                                              # the one host sync
        if deferred and got[0]:
            ov, oi, cnt, full = attempt(False)
            got = flags.tolist()
        if stats is not None:
            stats["margin_mean"] = float(cnt.float().mean())
            stats["uncertified_rows"] = int(full.sum())
        if got[1]:                                                        # a handful of rows at most: every fp32 score kept
            rows = torch.nonzero(full).flatten().int()
            fv, fi = dense_rows_topk(users_f32, H, items_f32, N, tag_bits, row_bits, hist_ptr, hist_items, rows, k)
            ov[rows.long()], oi[rows.long()] = fv, fi
        return ov, oi

    if defer:
        return ov, oi, finish
    return finish()


MEAN_MAX_PATTERNS = 32     # distinct tag words of a catalog the average-mode decode takes: one bit of a row-bits word each


def tag_patterns(tag_bits):
    """The pattern table of catalog_topk_mean: (words [P] int32: the distinct tag words of the catalog, pattern_bits [N] int32 =
    1 << (position of tag_bits[n] in words)).  tag_bits None (no tag table: every item carries bit 31): ([bit 31], None).
    Plain torch on whatever device tag_bits lives on; once per (item table, tags)."""
    if tag_bits is None:
        return torch.tensor([-(1 << 31)], dtype=torch.int32), None
    words, pid = torch.unique(tag_bits, return_inverse=True)
    if words.numel() > MEAN_MAX_PATTERNS:
        raise ValueError(f"split_mode=average: the catalog holds {words.numel()} distinct tag words, the fused decode takes at most "
                         f"{MEAN_MAX_PATTERNS}; rank such a catalog through predict() and the collector's dense average branch")
    bits = torch.ones_like(pid, dtype=torch.int64) << pid.long()
    return words.to(torch.int32), torch.where(bits >= (1 << 31), bits - (1 << 32), bits).to(torch.int32).contiguous()


def mean_rows_dense_topk(heads_f32, items_f32, n_items, tag_bits, row_bits, hist_ptr, hist_items, users, k):
    """Exact top-k (value desc, index asc) of the MEAN over finite heads for the users `users` (int32 [F]) with every item's mean
    kept: `mhr_catalog_mean_rows_dense` (pad / history / tag / row-bit masks as in the reference, items masked in every head at
    0.0 - collector.py:227-230) + the exact select over the whole row.  heads_f32 [B, H, D], items_f32 [N, D] fp32 normalised.
    -> (values [F, k] f32, indices [F, k] i64)."""
    B, H, D = heads_f32.shape
    N, dev = int(n_items), heads_f32.device
    users = users.to(torch.int32).contiguous()
    F_ = users.numel()
    ov = torch.empty(F_, k, dtype=torch.float32, device=dev)
    oi = torch.empty(F_, k, dtype=torch.int64, device=dev)
    for r0 in range(0, F_, DENSE_ROWS_CHUNK):                              # one scratch row per USER: the budget of dense_rows_topk
        r1 = min(F_, r0 + DENSE_ROWS_CHUNK)
        val = torch.empty(r1 - r0, N, dtype=torch.float32, device=dev)
        idx = torch.empty(r1 - r0, N, dtype=torch.int32, device=dev)
        cnt = torch.empty(r1 - r0, dtype=torch.int32, device=dev)
        _timed_call("mhr_catalog_mean_rows_dense", heads_f32.data_ptr(), items_f32.data_ptr(), D, N, users[r0:r1].data_ptr(), r1 - r0, H,
                    _ptr(tag_bits), row_bits.data_ptr(), _ptr(hist_ptr), _ptr(hist_items), val.data_ptr(), idx.data_ptr(),
                    cnt.data_ptr(), _stream())
        fv, fi, _, _ = topk_select((val, idx, cnt), N, k)
        ov[r0:r1], oi[r0:r1] = fv, fi
    return ov, oi


def catalog_topk_mean(heads_f32, items_bf, items_f32, tag_bits, row_bits, hist_ptr, hist_items, k, patterns=None, n_items=None,
                      stats=None, target=None):
    """split_mode = average without a [B, H, N] tensor: per-user top-k of the mean over FINITE heads of the fp32 scores (reference
    collector.py:227-230 on the masks of hstu.py:982-1015 and trainer.py:724-726), ranked (fp32 value desc, index asc).
    Head h is finite for item n iff n is not the pad id, not in the history and row_bits[b,h] & tag_bits[n] != 0: the finite set
    depends on n only through its tag word w, and the dot product is linear, so mean(b, n) = <q[b,w], i[n]> with q[b,w] the mean of
    the heads live for w.  The decode is therefore catalog_topk_exact's, single-headed, with P = (distinct tag words) query rows per
    user (`mhr_head_mean_queries`), each restricted to the items of its word by a one-hot pattern word per item in place of
    tag_bits and 1 << p per query row in place of row_bits; the candidates are re-scored with the reference's own arithmetic
    (`mhr_rescore_mean_f32`: H fp32 dots, finite ones summed, / count) and the P disjoint lists of a user merged.
    Two reference quirks: count + 1e-8 == count in fp32 (count >= 1), and an item masked in EVERY head scores 0 / 1e-8 = 0, not
    -inf, so it outranks negative means.  The merged list of a user is therefore trusted only when its k-th value is > 0; users
    where it is not (small catalogs), and users with an uncertified row, are re-ranked from every item's mean
    (`mhr_catalog_mean_rows_dense` + the exact select), zeros included.  Ties of exactly equal means ACROSS two patterns come out
    in pattern order (the merge's rule), within a pattern and on the dense path by ascending index.
    heads_f32 [B, H, D] fp32 normalised, items_bf [>= N, D] bf16 / items_f32 [N, D] fp32 normalised, tag_bits [N] int32 or None,
    row_bits [B*H] int32, history CSR over the B users; patterns: tag_patterns(tag_bits) (computed here when None).
    Sizes: P <= 32 (tag_patterns), P * k <= 8192 (the merge), H * D <= 16000 (the dense repair keeps a user's head rows in LDS).
    ONE host read per call on the streaming path (the bf16 pass's flag, the uncertified flag and the per-user flags together);
    a second one only when the bf16 pass's thresholds came up short and it is repeated.
    stats: patterns, margin_mean, uncertified_rows, dense_users (the list of re-ranked users).  -> (values [B, k] f32, indices [B, k] i64)."""
    _chk(heads_f32, "heads_f32", torch.float32)
    _chk(items_f32, "items_f32", torch.float32)
    B, H, D = heads_f32.shape
    N = items_f32.shape[0] if n_items is None else int(n_items)
    dev = heads_f32.device
    words, pattern_bits = tag_patterns(tag_bits) if patterns is None else patterns
    words = words.to(dev).contiguous()
    P = words.numel()
    if (pattern_bits is None) != (tag_bits is None) or (pattern_bits is None and P != 1):
        raise ValueError("catalog_topk_mean: patterns must come from tag_patterns(tag_bits)")
    q = torch.empty(B * P, D, dtype=torch.float32, device=dev)
    q_bits = torch.empty(B * P, dtype=torch.int32, device=dev)
    _timed_call("mhr_head_mean_queries", heads_f32.data_ptr(), row_bits.data_ptr(), words.data_ptr(), B, H, P, D,
                0 if pattern_bits is None else 1, q.data_ptr(), q_bits.data_ptr(), _stream())
    # |q| <= 1 (a mean of unit vectors), so the bf16 scorer's error bound 2^-8 holds for <q_bf16, i_bf16> as it does for a head row;
    # the fp32 difference between <q, i> and the mean of the H dots (about H * 2^-24) fits in the bound's slack (2^-8 is reached
    # only when every component's rounding error has the sign of the other operand's component)
    q_bf = q.to(torch.bfloat16)
    k2 = _margin_slots(N, k, D)
    deferred = decode_path(D, q_bf.dtype, items_bf.dtype) == "stream" and N > 4096 and stats is None
    flags = torch.empty(2, dtype=torch.int32, device=dev)
    n_rows = B * P

    def rescore(bi, cnt, rv, ri):
        _timed_call("mhr_rescore_mean_f32", heads_f32.data_ptr(), items_f32.data_ptr(), D, N, H, P, _ptr(tag_bits), row_bits.data_ptr(),
                    bi.data_ptr(), n_rows, k2, cnt.data_ptr(), rv.data_ptr(), ri.data_ptr(), _stream())

    def attempt(defer):
        ov, oi, cnt, full = _exact_attempt(q_bf, P, items_bf, N, pattern_bits, q_bits, hist_ptr, hist_items, k, k2, flags, defer, stats,
                                           target, rescore)
        if P > 1:                      # the P lists of a user hold disjoint item sets: the merge only merges
            mi, mv, _, uniq = multihead_merge_dedup(ov.view(B, P, k), oi.view(B, P, k), B, P, k)
            short = uniq < k           # (-inf completions of short lists may repeat an id; such a list ends <= 0 anyway)
        else:
            mv, mi, short = ov, oi, torch.zeros(B, dtype=torch.bool, device=dev)
        # a user is re-ranked densely when a row of his is uncertified or his k-th mean is not > 0: then items masked in every
        # head (mean 0 in the reference) belong in his list
        dense = full.view(B, P).any(dim=1) | short | ~(mv[:, k - 1] > 0)
        return mv, mi, cnt, full, dense

    mv, mi, cnt, full, dense = attempt(deferred)
    got = torch.cat([flags, dense.to(torch.int32)]).tolist()                  # the one host sync
    if deferred and got[0]:
        mv, mi, cnt, full, dense = attempt(False)
        got = torch.cat([flags, dense.to(torch.int32)]).tolist()
    users_f = [b for b in range(B) if got[2 + b]]
    if stats is not None:
        stats.update(patterns=P, margin_mean=float(cnt.float().mean()), uncertified_rows=int(full.sum()), dense_users=users_f)
    if users_f:
        users_t = torch.tensor(users_f, dtype=torch.int32, device=dev)
        fv, fi = mean_rows_dense_topk(heads_f32, items_f32, N, tag_bits, row_bits, hist_ptr, hist_items, users_t, k)
        mv[users_t.long()], mi[users_t.long()] = fv, fi
    return mv, mi


def multihead_merge_dedup(vals, idx, B, H, k):
    dev = vals.device
    out_idx = torch.empty(B, k, dtype=torch.int64, device=dev)
    out_val = torch.empty(B, k, dtype=torch.float32, device=dev)
    out_src = torch.empty(B, k, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    lib.call("mhr_multihead_merge_dedup", vals.data_ptr(), idx.data_ptr(), B, H, k, out_idx.data_ptr(), out_val.data_ptr(),
             out_src.data_ptr(), status.data_ptr(), _stream())
    return out_idx, out_val, out_src, status


def hit_matrix(topk_idx, positives, n_pos):
    B, k = topk_idx.shape
    hit = torch.empty(B, k, dtype=torch.uint8, device=topk_idx.device)
    lib.call("mhr_hit_matrix", topk_idx.data_ptr(), B, k, positives.data_ptr(), positives.stride(0), n_pos, hit.data_ptr(),
             _stream())
    return hit


# ------------------------------------------------------------------------------------------------
# streaming evaluation metrics
# ------------------------------------------------------------------------------------------------
METRIC_COLUMNS = ("recall", "ndcg", "hit", "mrr", "map", "precision")     # the column order of mhr_eval_metric_sums
METRIC_LIMITS = dict(K=2048, n_pred=16, n_topk=16, n_groups=32, n_tags=32)
_METRIC_CACHE = {}


def eval_metric_sums_workspace_bytes(B, n_pred, n_groups, n_topk):
    n = lib.load().mhr_eval_metric_sums_workspace_bytes(int(B), int(n_pred), int(n_groups), int(n_topk))
    if n < 0:
        raise ValueError(f"eval_metric_sums: sizes outside the kernel's limits {METRIC_LIMITS} "
                         f"(B={B}, n_pred={n_pred}, n_groups={n_groups}, n_topk={n_topk})")
    return n


def _metric_cached(key, make):
    v = _METRIC_CACHE.get(key)
    if v is None:
        if len(_METRIC_CACHE) >= 64:
            _METRIC_CACHE.clear()
        v = _METRIC_CACHE[key] = make()
    return v


def eval_metric_sums(topk_idx, positives, pos_len, pred, topk, group_bits, n_groups, sums, counts, item_tag_bits=None,
                     n_tags=0, entropy=None):
    """One launch pair per batch: sums [n_pred, n_groups, 6, n_topk] f64 (columns METRIC_COLUMNS), counts [n_pred, n_groups] i64
    and entropy [n_topk] f64 (with item_tag_bits [N] int32 words, bit c = tag c) get the batch's users ADDED - the caller owns
    and zeroes the accumulators.  topk_idx [B, K] i64, positives [B, >= max(pred) + 1] i64, pos_len [B, >= max(pred) + 1] i32,
    group_bits [B, n_pred] i32 words; pred / topk: host lists.  The discount tables and the workspace are cached per shape."""
    import ctypes
    _chk(topk_idx, "topk_idx", torch.int64)
    _chk(pos_len, "pos_len", torch.int32)
    _chk(group_bits, "group_bits", torch.int32)
    _chk(sums, "sums", torch.float64)
    _chk(counts, "counts", torch.int64)
    if positives.dtype != torch.int64 or positives.stride(1) != 1 or not positives.is_cuda:
        raise TypeError("positives: expected int64 rows on the GPU")
    B, K = topk_idx.shape
    n_pred, n_topk = len(pred), len(topk)
    dev = topk_idx.device
    assert tuple(group_bits.shape) == (B, n_pred) and positives.shape[0] == B and pos_len.shape[0] == B
    assert min(positives.shape[1], pos_len.shape[1]) > max(pred), "eval_metric_sums: positives / pos_len hold fewer than max(pred) + 1 columns"
    assert sums.numel() == n_pred * n_groups * len(METRIC_COLUMNS) * n_topk and counts.numel() == n_pred * n_groups
    if (item_tag_bits is None) != (entropy is None):
        raise ValueError("eval_metric_sums: item_tag_bits and entropy are given together or not at all")
    if entropy is not None:
        _chk(item_tag_bits, "item_tag_bits", torch.int32)
        _chk(entropy, "entropy", torch.float64)
        assert entropy.numel() == n_topk
    nbytes = eval_metric_sums_workspace_bytes(B, n_pred, n_groups, n_topk)

    def tables():
        d = 1.0 / torch.log2(torch.arange(2, K + 2, dtype=torch.float64))
        return torch.stack((d, torch.cumsum(d, 0))).to(dev)
    disc = _metric_cached(("disc", dev, K), tables)
    ws = _metric_cached(("ws", dev, nbytes), lambda: torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev))
    pred_c, topk_c = _metric_cached(("lists", tuple(pred), tuple(topk)),
                                    lambda: ((ctypes.c_int32 * n_pred)(*pred), (ctypes.c_int32 * n_topk)(*topk)))
    _timed_call("mhr_eval_metric_sums", topk_idx.data_ptr(), B, K, positives.data_ptr(), positives.stride(0), pos_len.data_ptr(),
                pos_len.stride(0), ctypes.addressof(pred_c), n_pred, ctypes.addressof(topk_c), n_topk, disc[0].data_ptr(),
                disc[1].data_ptr(), group_bits.data_ptr(), int(n_groups), _ptr(item_tag_bits),
                0 if item_tag_bits is None else item_tag_bits.numel(), int(n_tags), sums.data_ptr(), counts.data_ptr(),
                _ptr(entropy), ws.data_ptr(), _stream())


# ------------------------------------------------------------------------------------------------
# catalog exposure: item histogram -> coverage / popularity / tail / entropy / Gini sums
# ------------------------------------------------------------------------------------------------
EXPOSURE_COLUMNS = ("recommended", "popularity", "tail", "gini")          # the columns of mhr_exposure_finalize's out_int
EXPOSURE_LIMITS = dict(n_cuts=16, n_items=2 ** 31 - 1, users=2 ** 31 - 1)


def _exposure_cuts(cuts):
    import ctypes
    cuts = [int(c) for c in cuts]
    return _metric_cached(("cuts", tuple(cuts)), lambda: (ctypes.c_int32 * max(len(cuts), 1))(*cuts))


def exposure_accumulate(topk_idx, cuts, n_items, band_counts, bad):
    """One launch per batch: every (user, rank < cuts[-1]) of topk_idx [B, K] i64 adds 1 to band_counts[t][id], t = the first cut
    above the rank (cuts: ascending host list).  band_counts: int32, at least [len(cuts), n_items] words; bad: int32 [1], counts
    the ids outside [0, n_items) (they write nothing).  The caller owns and zeroes both."""
    import ctypes
    _chk(topk_idx, "topk_idx", torch.int64)
    _chk(band_counts, "band_counts", torch.int32)
    _chk(bad, "bad", torch.int32)
    if topk_idx.dim() != 2:
        raise ValueError("exposure_accumulate: topk_idx must be [B, K]")
    if band_counts.numel() < len(cuts) * int(n_items) or bad.numel() < 1:
        raise ValueError(f"exposure_accumulate: band_counts holds {band_counts.numel()} words, "
                         f"{len(cuts)} cuts x {n_items} items need {len(cuts) * int(n_items)}")
    B, K = topk_idx.shape
    _timed_call("mhr_exposure_accumulate", topk_idx.data_ptr(), B, K, ctypes.addressof(_exposure_cuts(cuts)), len(cuts),
                int(n_items), band_counts.data_ptr(), bad.data_ptr(), _stream())


def exposure_finalize_workspace_bytes(n_cuts, n_items, max_count):
    n = lib.load().mhr_exposure_finalize_workspace_bytes(int(n_cuts), int(n_items), int(max_count))
    if n < 0:
        raise ValueError(f"exposure_finalize: sizes outside the kernel's limits {EXPOSURE_LIMITS} "
                         f"(n_cuts={n_cuts}, n_items={n_items}, users={max_count})")
    return n


def exposure_finalize(band_counts, n_cuts, n_items, max_count, k_max, out_int, out_f64, bad, item_pop=None, item_tail=None):
    """out_int [n_cuts, 4] i64 (columns EXPOSURE_COLUMNS) and out_f64 [n_cuts] f64 (sum c ln c) from the histogram of
    `exposure_accumulate`; max_count = the users accumulated, k_max = the largest cut, item_pop [n_items] i64 / item_tail
    [n_items] u8 optional.  Counts above max_count add to bad.  The workspace is cached per size."""
    _chk(band_counts, "band_counts", torch.int32)
    _chk(out_int, "out_int", torch.int64)
    _chk(out_f64, "out_f64", torch.float64)
    _chk(bad, "bad", torch.int32)
    if band_counts.numel() < int(n_cuts) * int(n_items) or out_int.numel() < 4 * int(n_cuts) or out_f64.numel() < int(n_cuts):
        raise ValueError("exposure_finalize: band_counts / out_int / out_f64 are smaller than n_cuts x n_items / n_cuts x 4 / n_cuts")
    if item_pop is not None:
        _chk(item_pop, "item_pop", torch.int64)
    if item_tail is not None:
        _chk(item_tail, "item_tail", torch.uint8)
    for t, what in ((item_pop, "item_pop"), (item_tail, "item_tail")):
        if t is not None and t.numel() != int(n_items):
            raise ValueError(f"exposure_finalize: {what} holds {t.numel()} entries, n_items = {n_items}")
    nbytes = exposure_finalize_workspace_bytes(n_cuts, n_items, max_count)
    dev = band_counts.device
    ws = _metric_cached(("ws", dev, nbytes), lambda: torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev))
    _timed_call("mhr_exposure_finalize", band_counts.data_ptr(), int(n_cuts), int(n_items), _ptr(item_pop), _ptr(item_tail),
                int(max_count), int(k_max), out_int.data_ptr(), out_f64.data_ptr(), bad.data_ptr(), ws.data_ptr(), _stream())
