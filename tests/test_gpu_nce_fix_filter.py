"""The filtered false-negative bit table (mhr_nce_fix_bits_filtered: norm pass, 64-column prefix pass, exact pass over the
survivors) against the exhaustive kernel (mhr_nce_fix_bits) on the same inputs, through the C ABI: fix_any, slot_of_row and
every word of every flagged tile group must be EQUAL BIT FOR BIT (words of unflagged groups are unspecified: include/mhr.h).
Reference semantics: model/IDNet/hstu.py:611-613 (cos(target, negative) > nce_thres).

Cases: the cfg1 shape with seeded random rows and ~2 % planted hits; a small adversarial pool (targets planted in the pool,
near-duplicates whose cosine straddles thres within +-1e-3 with the whole difference inside / outside the prefix columns,
rows with all / none of their mass in the prefix, an all-zero target row) with unit-norm and x3-scaled negatives, thres in
{0.99, 0.5, 0.0, -1.0}, fp32 and bf16 targets, with and without a row list, n_neg = 2100 (neither whole tiles nor whole tile
groups), D = 256 and 128; and a pool of 8192 copies of one target row (every unit a candidate; its time is printed)."""
import os
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
CODE = os.path.join(ROOT, "multi-head-recommendation-with-human-priors_amd", "code")
KP = 64                                  # prefix columns of the filter (csrc/nce.hip: FIX_KPS * 16)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if CODE not in sys.path:
        sys.path.insert(0, CODE)
    import mhr_amd  # noqa: F401
    from mhr_amd import ops as _ops
    return _ops


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def _near(t, cos, cols, g):
    """Unit rows at cosine `cos` [n] to the unit rows t [n, D], differing from cos * t only in the columns `cols`."""
    e = torch.zeros_like(t)
    e[:, cols] = torch.randn(t.shape[0], cols.numel(), generator=g, dtype=t.dtype)
    ts = torch.zeros_like(t)
    ts[:, cols] = t[:, cols]
    e = e - (e * ts).sum(-1, keepdim=True) / (ts * ts).sum(-1, keepdim=True).clamp_min(1e-30) * ts       # e . t = 0, e inside cols
    delta = (1.0 / cos ** 2 - 1.0).sqrt()[:, None]
    return _unit(t + delta * _unit(e))


def _both(ops, p_rows, negs, n_neg, thres, mask):
    """-> [(fix_words, fix_any, slot_of_row)] of the exhaustive and the filtered entry, plus the filtered call's unit count."""
    from mhr_amd import lib
    dev = negs.device
    G, n_pad, D = negs.shape
    assert n_pad == (n_neg + 31) // 32 * 32
    n_p_rows = p_rows.shape[0]
    rp_pad = (n_p_rows + 255) // 256 * 256
    n_tiles = n_pad // 32
    row_list = n_list = None
    if mask is not None:
        ar = torch.arange(n_p_rows, dtype=torch.int32, device=dev)
        row_list, _, _, n_list = ops.token_compact(mask.contiguous(), ar[None].expand(G, -1).contiguous(), ar, ar, tok_cap=rp_pad)
    ptr = lambda t: 0 if t is None else t.data_ptr()     # noqa: E731
    dt = lib.BF16 if p_rows.dtype == torch.bfloat16 else lib.F32
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    n_units = None
    for filtered in (False, True):
        words = torch.full((G, n_tiles, rp_pad), 0x5A5A5A5A, dtype=torch.int32, device=dev)      # unflagged words: unspecified
        fix_any = torch.zeros(G, rp_pad, dtype=torch.int32, device=dev)
        slot = torch.zeros(G, n_p_rows, dtype=torch.int32, device=dev) if mask is not None else None
        args = (p_rows.data_ptr(), dt, n_p_rows, negs.data_ptr(), n_neg, D, G, float(thres), words.data_ptr(), ptr(row_list),
                ptr(n_list), ptr(slot), fix_any.data_ptr())
        if filtered:
            nb = lib.load().mhr_nce_fix_bits_filtered_workspace_bytes(n_p_rows, n_neg, G)
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            lib.call("mhr_nce_fix_bits_filtered", *args, ws.data_ptr(), nb, st)
            torch.cuda.synchronize()
            n_units = int(ws[:4].view(torch.int32).item())
        else:
            lib.call("mhr_nce_fix_bits", *args, st)
            torch.cuda.synchronize()
        outs.append((words, fix_any, slot))
    return outs, n_units


def _assert_same(outs, n_tiles):
    (wa, aa, sa), (wb, ab, sb) = outs
    assert torch.equal(aa, ab), "fix_any differs"
    if sa is not None:
        assert torch.equal(sa, sb), "slot_of_row differs"
    shift = 0
    while ((n_tiles + (1 << shift) - 1) >> shift) > 32:
        shift += 1
    grp = (torch.arange(n_tiles, device=aa.device) >> shift)[None, :, None]              # tile -> group bit of fix_any
    flagged = ((aa[:, None, :] >> grp) & 1).bool()                                        # [G, n_tiles, rp_pad]
    assert torch.equal(wa[flagged], wb[flagged]), "a word of a flagged tile group differs"
    return int(flagged.sum()), int((wa[flagged] != 0).sum())


def _adversarial(D, n_rows, n_neg, G, thres, scale, seed):
    """Targets (fp32, not normalised) and pools [G, n_pad, D] bf16 holding every construction of the module docstring."""
    g = torch.Generator().manual_seed(seed)
    n_pad = (n_neg + 31) // 32 * 32
    t = torch.randn(n_rows, D, generator=g, dtype=torch.float64)
    t[10:20, KP:] = 0.0                                  # all mass in the prefix
    t[20:30, :KP] = 0.0                                  # none there
    t[30:34] = t[30:34] * 1e-3                           # small rows (the kernels normalise)
    tn = _unit(t)
    t[5] = 0.0                                           # all-zero target row: NaN products, bits 0
    negs = _unit(torch.randn(G, n_pad, D, generator=g, dtype=torch.float64))
    negs[:, 100:110, KP:] = 0.0
    negs[:, 110:120, :KP] = 0.0
    negs[:, 100:120] = _unit(negs[:, 100:120])
    pre, rest = torch.arange(0, KP), torch.arange(KP, D)
    c = float(min(max(thres, -0.9), 0.999))              # straddled cosine (clamped where thres itself is not a cosine)
    for gi in range(G):
        src = torch.randint(0, n_rows, (160,), generator=g)
        src[src == 5] = 6
        cos = c + (torch.rand(64, generator=g, dtype=torch.float64) * 2 - 1) * 1e-3
        negs[gi, 200:232] = tn[src[:32]]                                                  # planted: cos = 1
        negs[gi, 300:364] = _near(tn[src[32:96]], cos.clamp(max=0.99999), pre, g)          # difference inside the prefix
        negs[gi, 400:464] = _near(tn[src[96:160]], cos.clamp(max=0.99999), rest, g)        # difference outside it
        negs[gi, n_pad - 40:n_pad - 8] = tn[src[:32]]                                     # hits in the last, partial group
    return t.float(), (negs * scale).to(torch.bfloat16)


@pytest.mark.parametrize("with_list", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("thres", [0.99, 0.5, 0.0, -1.0])
@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_filtered_table_equals_exhaustive_adversarial(ops, scale, thres, dtype, with_list):
    D, n_rows, n_neg, G = 256, 300, 2100, 2
    t, negs = _adversarial(D, n_rows, n_neg, G, thres, scale, seed=7)
    mask = None
    if with_list:
        mask = (torch.rand(G, n_rows, generator=torch.Generator().manual_seed(3)) < 0.6)
        mask[:, :40] = True
        mask = mask.cuda()
    outs, n_units = _both(ops, t.to(dtype).cuda(), negs.cuda(), n_neg, thres, mask)
    n_flag, n_hit = _assert_same(outs, negs.shape[1] // 32)
    cap = G * (512 // 32) * (negs.shape[1] // 32)
    print(f"scale={scale} thres={thres} {dtype} list={with_list}: units {n_units}/{cap} flagged words {n_flag} non-zero {n_hit}")
    assert 0 < n_hit and 0 <= n_units <= cap             # the planted targets are hits at every thres: the check is not vacuous
    if thres <= 0.0 and scale == 1.0 and not with_list:
        assert n_units > cap // 2                        # nothing to reject there: still identical


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_filtered_table_equals_exhaustive_dim128(ops, dtype):
    t, negs = _adversarial(128, 300, 2100, 2, 0.99, 1.0, seed=11)
    outs, n_units = _both(ops, t.to(dtype).cuda(), negs.cuda(), 2100, 0.99, None)
    n_flag, n_hit = _assert_same(outs, negs.shape[1] // 32)
    print(f"D=128 {dtype}: units {n_units} flagged words {n_flag} non-zero {n_hit}")
    assert n_hit > 0


@pytest.mark.parametrize("with_list", [False, True])
def test_filtered_table_equals_exhaustive_cfg1_shape(ops, with_list):
    """cfg1: 4 prior categories, 8192 negatives per pool, D = 256, 4672 target rows (bf16), thres = 0.99; 2 % of the target
    rows are also drawn into every pool."""
    D, n_rows, n_neg, G = 256, 4672, 8192, 4
    g = torch.Generator().manual_seed(2024)
    t = torch.randn(n_rows, D, generator=g)
    negs = _unit(torch.randn(G, n_neg, D, generator=g))
    for gi in range(G):
        src = torch.randperm(n_rows, generator=g)[: n_rows // 50]
        dst = torch.randperm(n_neg, generator=g)[: n_rows // 50]
        negs[gi, dst] = _unit(t[src])
    mask = (torch.rand(G, n_rows, generator=g) < 0.5).cuda() if with_list else None
    outs, n_units = _both(ops, t.bfloat16().cuda(), negs.bfloat16().cuda(), n_neg, 0.99, mask)
    n_flag, n_hit = _assert_same(outs, n_neg // 32)
    cap = G * (4864 // 32) * (n_neg // 32)
    print(f"cfg1 shape list={with_list}: units {n_units}/{cap} flagged words {n_flag} non-zero {n_hit}")
    assert n_hit >= (n_rows // 50) * G * (0.4 if with_list else 0.95)


def test_filtered_table_equals_exhaustive_all_duplicates(ops):
    """The worst case: every pool is 8192 copies of one target row, so every (fragment, tile) unit holding that row - and,
    at thres = -1, every unit - goes through the exact pass.  Correct, and no overflow; the times are printed."""
    D, n_rows, n_neg, G = 256, 4672, 8192, 4
    g = torch.Generator().manual_seed(5)
    t = torch.randn(n_rows, D, generator=g)
    negs = _unit(t[17])[None, None].expand(G, n_neg, D).contiguous()
    for thres in (0.99, -1.0):
        outs, n_units = _both(ops, t.bfloat16().cuda(), negs.bfloat16().cuda(), n_neg, thres, None)
        n_flag, n_hit = _assert_same(outs, n_neg // 32)
        cap = G * (4864 // 32) * (n_neg // 32)
        print(f"all duplicates thres={thres}: units {n_units}/{cap} flagged words {n_flag} non-zero {n_hit}")
        assert n_hit >= G * (n_neg // 32)
        if thres == -1.0:
            assert n_units == G * (4864 // 32 - (4864 - 4672) // 32) * (n_neg // 32) or n_units == cap

    from mhr_amd import lib
    dev = torch.device("cuda")
    p, n = t.bfloat16().cuda(), negs.bfloat16().cuda()
    words = torch.empty(G, n_neg // 32, 4864, dtype=torch.int32, device=dev)
    fix_any = torch.zeros(G, 4864, dtype=torch.int32, device=dev)
    nb = lib.load().mhr_nce_fix_bits_filtered_workspace_bytes(n_rows, n_neg, G)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    args = (p.data_ptr(), lib.BF16, n_rows, n.data_ptr(), n_neg, D, G, -1.0, words.data_ptr(), 0, 0, 0, fix_any.data_ptr())
    for name, extra in (("mhr_nce_fix_bits", ()), ("mhr_nce_fix_bits_filtered", (ws.data_ptr(), nb))):
        lib.call(name, *args, *extra, st)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            lib.call(name, *args, *extra, st)
        e1.record()
        torch.cuda.synchronize()
        print(f"all duplicates, thres = -1 (every unit a candidate): {name} {e0.elapsed_time(e1) / 3 * 1e3:.0f} us per call")
