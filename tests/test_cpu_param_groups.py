"""Per-group learning rate and weight decay in the fused AdamW, host side (no GPU): the C ABI of `mhr_adam_flat_groups` is
declared, exported and validates its arguments before any launch; FusedAdamW(param_groups=...) lays the segment tables out
without reordering anything, `None` is exactly the ungrouped optimizer, and the Trainer builds the groups from
`lr_mult_prefix` / `lr_mult_rate` under the reference's condition (both keys truthy)."""
import os
import sys

import pytest
import torch

from conftest import ROOT

CODE = os.path.join(ROOT, "multi-head-recommendation-with-human-priors_amd", "code")
if CODE not in sys.path:
    sys.path.insert(0, CODE)


@pytest.fixture(scope="module")
def dll():
    import __graft_entry__ as ge
    ge.build_hip_library()
    import mhr_amd  # noqa: F401
    from mhr_amd import lib
    return lib.load()


def test_the_grouped_entry_is_declared_exported_and_validates_on_the_host(dll):
    from mhr_amd import lib
    assert "mhr_adam_flat_groups" in lib.declared_symbols() and "mhr_adam_flat_groups" in lib.SIGNATURES
    assert lib.check_exports()
    assert len(lib.SIGNATURES["mhr_adam_flat_groups"]) == 21
    assert len(lib.SIGNATURES["mhr_adam_flat"]) == 17 and len(lib.SIGNATURES["mhr_adam_flat_scaled"]) == 18    # untouched
    P = 64                                     # dummy non-null pointer: a launch would fault on it, validation comes first
    f = dll.mhr_adam_flat_groups

    def call(w=P, g=P, m=P, v=P, n=8, step=1, w16=None, seg_off=P, seg_group=P, n_seg=1, chunk_seg=P, gconst=P, hist_len=64,
             n_groups=1, step_dev=None, scale_dev=None):
        rc = f(w, g, m, v, n, 1.0, 0.9, 0.999, 1e-8, step, w16, seg_off, seg_group, n_seg, chunk_seg, gconst, hist_len, n_groups,
               step_dev, scale_dev, None)
        return rc, dll.mhr_last_error()

    for kw, word in ((dict(w=None), b"w / g / m / v"), (dict(g=None), b"w / g / m / v"), (dict(m=None), b"w / g / m / v"),
                     (dict(v=None), b"w / g / m / v"), (dict(seg_off=None), b"seg_off"), (dict(seg_group=None), b"seg_group"),
                     (dict(chunk_seg=None), b"chunk_seg"), (dict(gconst=None), b"gconst"),
                     (dict(n=12), b"n=12"), (dict(n=-8), b"n=-8"), (dict(n_seg=0), b"n_seg=0"),
                     (dict(n_groups=0), b"n_groups=0"), (dict(n_groups=17), b"n_groups=17"), (dict(hist_len=0), b"hist_len=0"),
                     (dict(step=0), b"step=0"), (dict(w=72), b"16-byte"), (dict(v=68), b"16-byte"), (dict(w16=68), b"w_bf16")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg and b"adam_flat_groups" in msg, (kw, msg)
    # step < 1 is an error only when the step comes from the argument; an empty buffer is no launch
    rc, msg = call(step=0, step_dev=P, n=0)
    assert rc == 0, msg
    assert call(n=0)[0] == 0 and call(n=0, n_groups=16)[0] == 0


class Toy(torch.nn.Module):
    """5 parameters of 7, 45, 8, 3 and 64 elements: slots of 8, 48, 8, 8, 64 in the flat buffers (136 elements)."""
    def __init__(self):
        super().__init__()
        self.enc_a = torch.nn.Parameter(torch.randn(7))
        self.enc_b = torch.nn.Parameter(torch.randn(5, 9))
        self.head_a = torch.nn.Parameter(torch.randn(8))
        self.enc_c = torch.nn.Parameter(torch.randn(3))
        self.head_b = torch.nn.Parameter(torch.randn(8, 8))


def test_segment_tables_of_a_toy_module_for_two_prefix_lists(dll):
    from mhr_amd.optim import FusedAdamW
    # one listed group: enc_a, enc_b | head_a | enc_c | head_b
    opt = FusedAdamW(Toy(), lr=1e-3, weight_decay=0.01, param_groups=[{"prefixes": ["head_"], "lr_ratio": 5.0, "weight_decay": None}])
    assert [x[1] for x in opt.layout] == [7, 45, 8, 3, 64] and [x[0] for x in opt.layout] == ["enc_a", "enc_b", "head_a", "enc_c", "head_b"]
    seg_off, seg_group, chunk_seg = opt._seg_lists
    assert seg_off == [0, 56, 64, 72, 136] and seg_group == [0, 1, 0, 1] and chunk_seg == [0]
    assert opt._seg.seg_off.tolist() == seg_off and opt._seg.seg_off.dtype == torch.int64
    assert opt._seg.seg_group.tolist() == seg_group and opt._seg.seg_group.dtype == torch.int32
    assert opt._seg.chunk_seg.tolist() == chunk_seg and opt._seg.chunk_seg.dtype == torch.int32
    assert (opt._seg.n, opt._seg.n_seg, opt._seg.n_groups) == (136, 4, 2) and opt.flat_w.numel() == 136
    assert [g["names"] for g in opt.groups] == [["enc_a", "enc_b", "enc_c"], ["head_a", "head_b"]]
    assert [g["weight_decay"] for g in opt.groups] == [0.01, 0.01] and [g["lr_ratio"] for g in opt.groups] == [1.0, 5.0]
    assert [pg["lr"] for pg in opt.param_groups] == [1e-3, 1e-3 * 5.0]
    assert all(set(pg) == {"lr", "weight_decay", "lr_ratio", "names"} for pg in opt.param_groups)
    assert opt.gconst.shape == (64, 2, 4) and opt.hist.shape == (65, 4) and opt.ctrl.shape == (2,) and opt.ctrl.dtype == torch.int64
    # two listed groups; "enc_" comes first, so it wins over the later "enc_b" (first match); head_a matches nothing listed here
    # and stays in group 0; head_b is group 2
    opt = FusedAdamW(Toy(), lr=1e-3, weight_decay=0.01,
                     param_groups=[{"prefixes": ["enc_"], "lr_ratio": 0.5, "weight_decay": 0.0},
                                   {"prefixes": ["enc_b", "head_b"], "lr_ratio": 3.0}])
    seg_off, seg_group, chunk_seg = opt._seg_lists
    assert seg_off == [0, 56, 64, 72, 136] and seg_group == [1, 0, 1, 2] and chunk_seg == [0]
    assert [g["names"] for g in opt.groups] == [["head_a"], ["enc_a", "enc_b", "enc_c"], ["head_b"]]
    assert [g["weight_decay"] for g in opt.groups] == [0.01, 0.0, 0.01]
    # consecutive parameters of one group merge: everything in one listed group is ONE segment; so is nothing matched
    opt = FusedAdamW(Toy(), param_groups=[{"prefixes": ["enc_", "head_"], "lr_ratio": 2.0}])
    assert opt._seg_lists == ([0, 136], [1], [0])
    opt = FusedAdamW(Toy(), param_groups=[{"prefixes": ["nothing"], "lr_ratio": 2.0}])
    assert opt._seg_lists == ([0, 136], [0], [0]) and opt.groups[1]["names"] == []
    opt = FusedAdamW(Toy(), param_groups=[])
    assert opt._seg_lists == ([0, 136], [0], [0]) and len(opt.groups) == 1
    with pytest.raises(ValueError):
        FusedAdamW(Toy(), param_groups=[{"prefixes": ["enc_"]}])
    with pytest.raises(ValueError):
        FusedAdamW(Toy(), param_groups=[{"prefixes": [f"p{k}"], "lr_ratio": 1.0} for k in range(16)])      # 17 with group 0


def test_chunk_table_names_the_segment_that_holds_each_chunk_start(dll):
    from mhr_amd import ops
    # a boundary exactly on the chunk edge: chunk 1 starts in the segment that BEGINS there
    assert ops.adam_chunk_segments([0, 8, 8192, 8200]) == [0, 2]
    # an empty segment is never a chunk's first; a segment spanning two chunks holds both starts
    assert ops.adam_chunk_segments([0, 8192, 8192, 24584]) == [0, 2, 2, 2]
    assert ops.adam_chunk_segments([0, 0]) == []
    off, grp, chunk = ops.adam_group_segments([8190, 5, 8192], [0, 1, 1])
    assert (off, grp, chunk) == ([0, 8192, 16392], [0, 1], [0, 1, 1])
    for bad_off, bad_grp, n_g in (([0, 4, 8], [0, 0], 1), ([0, 16, 8], [0, 0], 1), ([8, 16], [0], 1), ([0, 8], [1], 1), ([0, 8], [0], 17),
                                  ([0, 8], [0, 0], 1), ([0], [], 1)):
        with pytest.raises(ValueError):
            ops.adam_group_tables(bad_off, bad_grp, n_g, "cpu")


def test_no_groups_is_todays_optimizer_nothing_new_allocated_same_state_keys(dll):
    from mhr_amd.optim import FusedAdamW
    base = FusedAdamW(Toy(), lr=1e-3, weight_decay=0.01)
    none = FusedAdamW(Toy(), lr=1e-3, weight_decay=0.01, param_groups=None)
    for o in (base, none):
        assert o.groups is None and o.param_groups == [{"lr": 1e-3}]
        assert not any(hasattr(o, a) for a in ("gconst", "_gconst_host", "_seg", "_seg_lists", "_table_group"))
        assert o.hist.shape == (65, 4) and o._hist_host.shape == (65, 4) and o._hist_ring.shape == (64, 65, 4)
        assert o._consts_dev is o.hist and o._consts_host is o._hist_host                   # aliases, not buffers
        assert sorted(o.state_dict()) == ["flat_m", "flat_v", "layout", "pad", "step"]
    assert sorted(base.__dict__) == sorted(none.__dict__)
    grouped = FusedAdamW(Toy(), lr=1e-3, weight_decay=0.01, param_groups=[{"prefixes": ["head_"], "lr_ratio": 5.0, "weight_decay": 0.0}])
    sd = grouped.state_dict()
    assert sorted(sd) == ["flat_m", "flat_v", "groups", "layout", "pad", "step"]
    assert sd["groups"] == [{"lr_ratio": 1.0, "weight_decay": 0.01, "names": ["enc_a", "enc_b", "enc_c"]},
                            {"lr_ratio": 5.0, "weight_decay": 0.0, "names": ["head_a", "head_b"]}]
    assert sd["layout"] == base.state_dict()["layout"]                                      # nothing is reordered
    # a state with the record loads, into a grouped and into an ungrouped optimizer; a state without it loads into a grouped one
    sd["step"] = 3
    grouped.load_state_dict(sd)
    base.load_state_dict(sd)
    grouped.load_state_dict(none.state_dict())
    assert grouped.step_count == 0 and base.step_count == 3


def test_per_step_constants_are_one_adam_consts_row_per_group(dll):
    """The host half of the upload: the rows a step pushes are `mhr_adam_consts` of (lr * ratio, weight decay) per group, the
    table's row in `hist` is its group's, and the other groups' lr is written back for logging."""
    import ctypes
    from mhr_amd.optim import FusedAdamW

    class WithTable(Toy):
        def __init__(self):
            super().__init__()
            self.item_embedding = torch.nn.Embedding(10, 8)

    opt = FusedAdamW(WithTable(), lr=1e-3, weight_decay=0.01,
                     param_groups=[{"prefixes": ["item_embedding"], "lr_ratio": 4.0, "weight_decay": 0.0},
                                   {"prefixes": ["head_"], "lr_ratio": 0.25}])
    assert opt._table_group == 1 and opt.groups[1]["names"] == ["item_embedding.weight"]
    opt._push_consts(7, 2e-3, ctrl=(11, 7))
    want = (ctypes.c_float * 4)()
    for k, (lr, wd) in enumerate(((2e-3, 0.01), (2e-3 * 4.0, 0.0), (2e-3 * 0.25, 0.01))):
        assert dll.mhr_adam_consts(lr, 0.9, 0.999, 1e-8, wd, 7, want) == 0
        assert opt.gconst[7, k].tolist() == list(want), k
        if k == 1:
            assert opt.hist[7].tolist() == list(want)
    assert opt.ctrl.tolist() == [11, 7]
    assert [pg["lr"] for pg in opt.param_groups[1:]] == [2e-3 * 4.0, 2e-3 * 0.25]
    assert float(opt.gconst.abs().sum()) == float(opt.gconst[7].abs().sum())                # one row written


def _trainer(**over):
    import REC  # noqa: F401
    import mhr_amd.synth as synth
    from REC.config.configurator import Config, apply_run_fixups
    from REC.trainer import Trainer
    from REC.utils import get_model
    kw = dict(MAX_ITEM_LIST_LENGTH=12, n_layers=1, n_heads=1, item_embedding_size=16, hstu_embedding_size=16, num_negatives=64,
              device="cpu", total_iters=10, eval_interval=0, checkpoint_dir=None, save_model_note="t", scheduler_args=None)
    kw.update(over)
    cfg = apply_run_fixups(Config(config_dict=synth.base_config(**kw)))
    data = synth.SyntheticData(cfg, 200, torch.device("cpu"))
    cfg["int_to_category"] = data.int_to_category
    tr = Trainer(cfg)
    tr.setup_model(get_model("HSTU")(cfg, data))
    return tr


def test_trainer_builds_the_groups_from_lr_mult_prefix_and_rate(dll):
    tr = _trainer(lr_mult_prefix=['item_embedding'], lr_mult_rate=5.0)
    opt = tr.optimizer
    assert len(opt.groups) == 2 and opt.groups[1]["lr_ratio"] == 5.0
    assert opt.groups[1]["names"] == ["item_embedding.weight"] and opt._table_group == 1
    assert opt.groups[1]["weight_decay"] == opt.groups[0]["weight_decay"] == tr.optim_args["weight_decay"]
    assert opt.param_groups[1]["lr"] == tr.optim_args["learning_rate"] * 5.0
    assert opt._seg_lists[1] == [0]                                   # the table is not in the flat buffer: one segment
    for over in ({}, dict(lr_mult_prefix=None, lr_mult_rate=5.0), dict(lr_mult_prefix=[], lr_mult_rate=5.0),
                 dict(lr_mult_prefix=['item_embedding'], lr_mult_rate=None), dict(lr_mult_prefix=['item_embedding'], lr_mult_rate=0)):
        assert _trainer(**over).optimizer.groups is None, over
    # a rate of 1.0 still builds the group (the reference's condition is truthiness)
    opt = _trainer(lr_mult_prefix=['item_embedding', 'position_embedding'], lr_mult_rate=1.0).optimizer
    assert len(opt.groups) == 2 and opt.groups[1]["lr_ratio"] == 1.0 and len(opt.groups[1]["names"]) >= 2
