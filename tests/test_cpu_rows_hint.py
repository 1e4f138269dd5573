"""The batchers' host-side row capacity for the packed encoder rows (`packed_rows`, REC/data/batcher.py): every batch carries
`rows_cap` = mhr_amd.synth.rows_capacity of its valid context positions, computed from host copies of the window lengths and
never from the batch's tensors - so the checks below count the mask / item_seq the batcher made and compare.  Data parallel:
all ranks carry the same capacity in a step (the maximum over the ranks' slices).  CPU only."""
import os
import sys

import pytest
import torch

from conftest import ROOT
from rows_hint_data import B, BUCKET, L, config_dict, make_data

CODE = os.path.join(ROOT, "multi-head-recommendation-with-human-priors_amd", "code")
if CODE not in sys.path:
    sys.path.insert(0, CODE)


def _cfg(**kw):
    from REC.config.configurator import Config
    return Config(config_dict=config_dict(**kw))


@pytest.fixture(scope="module")
def store():
    from REC.data import SeqStore
    return SeqStore(*make_data())


def _cap(n_valid, b_step):
    from mhr_amd.synth import rows_capacity
    return rows_capacity(int(n_valid), n_rows=b_step * L, bucket=BUCKET)


def test_train_batches_carry_their_row_capacity(store):
    from REC.data import SeqTrainBatcher
    tb = SeqTrainBatcher(_cfg(packed_rows=True), store, seed=7, rows_bucket=BUCKET)
    seen, n = set(), 0
    for batch in tb:
        assert isinstance(batch, tuple) and len(batch) == 4
        items, neg, mask, tags = batch
        assert all(torch.is_tensor(t) for t in (items, neg, mask, tags)) and batch[2] is mask
        bs = mask.shape[0]
        want = _cap(mask[:, :L].sum(), bs)
        assert isinstance(batch.rows_cap, int) and batch.rows_cap == want and mask._mhr_rows_cap == want
        assert 0 < want < bs * L
        seen.add((bs, want))
        n += 1
    assert n == len(tb) and {b for b, _ in seen} == {B, 150 % B} and len({c for _, c in seen}) > 1, seen


def test_train_ranks_share_the_capacity_of_the_fullest_rank(store):
    from REC.data import SeqTrainBatcher
    cfg = _cfg(packed_rows=True)
    r0, r1 = (SeqTrainBatcher(cfg, store, seed=7, rank=r, world=2, rows_bucket=BUCKET) for r in (0, 1))
    steps, differ = 0, 0
    for b0, b1 in zip(r0, r1):
        bs = b0[2].shape[0]
        assert b1[2].shape[0] == bs
        n0, n1 = int(b0[2][:, :L].sum()), int(b1[2][:, :L].sum())
        assert b0.rows_cap == b1.rows_cap == _cap(max(n0, n1), bs)
        assert b0.rows_cap >= n0 and b0.rows_cap >= n1 and 0 < b0.rows_cap < bs * L
        assert b0[2]._mhr_rows_cap == b1[2]._mhr_rows_cap == b0.rows_cap
        differ += _cap(n0, bs) != _cap(n1, bs)
        steps += 1
    assert steps == len(r0) == len(r1) == 5
    assert differ > 0            # (the maximum matters: some step's ranks would have chosen different capacities on their own)


@pytest.mark.parametrize("phase", ["valid", "test"])
def test_eval_batches_carry_their_row_capacity(store, phase):
    from REC.data import SeqEvalBatcher
    eb = SeqEvalBatcher(_cfg(packed_rows=True), store, phase=phase, rows_bucket=BUCKET)
    n = 0
    for batch in eb:
        assert isinstance(batch, tuple) and len(batch) == 8
        item_seq = batch[1]
        bs = item_seq.shape[0]
        want = _cap((item_seq != 0).sum(), bs)
        assert batch.rows_cap == want and item_seq._mhr_rows_cap == want and 0 < want < bs * L
        n += 1
    assert n == len(eb)
    # two ranks: each its own users and its own capacity (eval steps issue no collective)
    for r in (0, 1):
        for batch in SeqEvalBatcher(_cfg(packed_rows=True), store, phase=phase, rank=r, world=2, rows_bucket=BUCKET):
            assert batch.rows_cap == _cap((batch[1] != 0).sum(), batch[1].shape[0])


@pytest.mark.parametrize("off", [{}, {"packed_rows": False}])
def test_without_the_key_nothing_changes(store, off):
    from REC.data import SeqEvalBatcher, SeqTrainBatcher
    plain = SeqTrainBatcher(_cfg(**off), store, seed=7)
    hinted = SeqTrainBatcher(_cfg(packed_rows=True), store, seed=7, rows_bucket=BUCKET)
    n = 0
    for a, b in zip(plain, hinted):
        assert isinstance(a, tuple) and len(a) == 4 and a.rows_cap is None and not hasattr(a[2], "_mhr_rows_cap")
        assert all(torch.equal(x, y) for x, y in zip(a, b))                 # the hint does not perturb the sampling
        n += 1
    assert n == len(plain)
    for a, b in zip(SeqEvalBatcher(_cfg(**off), store), SeqEvalBatcher(_cfg(packed_rows=True), store, rows_bucket=BUCKET)):
        assert len(a) == 8 and a.rows_cap is None and not hasattr(a[1], "_mhr_rows_cap")
        for x, y in zip(a, b):
            if isinstance(x, tuple):
                assert all(torch.equal(p, q) for p, q in zip(x, y))
            else:
                assert torch.equal(x, y)


def test_batch_rows_cap_counts_cpu_tensors_only(store):
    from mhr_amd.synth import rows_capacity
    from REC.data import SeqEvalBatcher, SeqTrainBatcher
    from REC.data.batcher import batch_rows_cap
    for items, neg, mask, tags in SeqTrainBatcher(_cfg(), store, seed=7):
        bs = mask.shape[0]
        assert batch_rows_cap(mask, L, bucket=BUCKET) == _cap(mask[:, :L].sum(), bs)
        assert batch_rows_cap(mask, L) == rows_capacity(int(mask[:, :L].sum()), n_rows=bs * L)
        assert batch_rows_cap(mask.to("meta"), L, bucket=BUCKET) is None      # "not on the CPU": counting would be a sync
    item_seq = next(iter(SeqEvalBatcher(_cfg(), store)))[1]
    assert batch_rows_cap(item_seq, L, bucket=BUCKET) == _cap((item_seq != 0).sum(), item_seq.shape[0])
    assert batch_rows_cap(item_seq.to("meta"), L) is None
