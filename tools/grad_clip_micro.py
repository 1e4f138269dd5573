"""Cost of gradient clipping at a config's real shapes (default cfg1): the flat gradient's length and the sparse row set of one
real training step, then HIP events around warmed launches of the squared-norm kernels and the coefficient launch, and the
whole replayed step with the key off and on.  Each launch is timed twice: on ONE buffer (what the step sees when the
gradient was just written and still sits in the 256 MB MALL) and rotating over copies that together exceed the MALL (what
HBM delivers).  Bytes are the algorithm's: every fp32 element of the flat gradient once; for the rows the ids (two reads of
8 bytes) and the segment-head rows once."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multi-head-recommendation-with-human-priors_amd", "code"))
import mhr_amd  # noqa: E402,F401
import mhr_amd.synth as synth  # noqa: E402
from mhr_amd import ops  # noqa: E402

HBM_GBS = 8000.0


def timed(fn, n_variants, reps):
    for i in range(3 * n_variants):
        fn(i % n_variants)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i % n_variants)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg1")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100, help="timed replayed steps per end-to-end measurement")
    ap.add_argument("--step-repeats", type=int, default=3, help="off/on pairs of the end-to-end measurement (0: skip)")
    args = ap.parse_args()
    import REC  # noqa: F401
    from REC.config.configurator import Config, apply_run_fixups
    from REC.trainer import Trainer
    from REC.utils import get_model
    dev = torch.device("cuda", 0)
    spec = synth.CONFIGS[args.config]
    cfgd = dict(spec["cfg"], device=dev, total_iters=30000, eval_interval=0, checkpoint_dir=None, save_model_note="micro",
                hip_graph=False, clip_grad_norm=1.0)
    cfg = apply_run_fixups(Config(config_dict=cfgd))
    data = synth.SyntheticData(cfg, spec["item_num"], dev, seed=2020)
    cfg["int_to_category"] = data.int_to_category
    torch.manual_seed(2020)
    model = get_model("HSTU")(cfg, data).to(dev)
    tr = Trainer(cfg)
    tr.setup_model(model)
    tr.train_step = 3000
    opt = tr.optimizer
    model.train()
    # one real step, minus zero_grad(): the gradients the clipped optimizer saw
    out = model(data.train_batch(cfg["train_batch_size"]))
    out["loss"].backward()
    opt.step()
    sg = model.sparse_grad
    torch.cuda.synchronize()
    n_flat, n_ids, D = opt.flat_g.numel(), sg.sorted_ids.numel(), sg.rows.shape[1]
    head = torch.ones_like(sg.sorted_ids, dtype=torch.bool)
    head[1:] = sg.sorted_ids[1:] != sg.sorted_ids[:-1]
    n_heads = int(head.sum())
    print(f"{args.config}: flat gradient {n_flat} fp32 ({n_flat * 4 / 1e6:.1f} MB); sparse rows {n_ids} x {D} "
          f"({n_ids * D * 4 / 1e6:.1f} MB), {n_heads} segment heads ({n_heads * D * 4 / 1e6:.1f} MB read); "
          f"grad_norm of the step {float(opt.grad_norm):.4f}")
    p_flat, p_rows = ops.grad_sqnorm_partials(n_flat), ops.grad_sqnorm_partials(n_ids, D)
    partials = torch.zeros(p_flat + p_rows, dtype=torch.float64, device=dev)
    state = torch.zeros(2, dtype=torch.float32, device=dev)
    mall = 256 << 20
    k_flat = mall // (n_flat * 4) + 2
    k_rows = mall // (n_ids * D * 4) + 2
    flats = [opt.flat_g] + [opt.flat_g.clone() for _ in range(k_flat - 1)]
    rows = [sg.rows] + [sg.rows.clone() for _ in range(k_rows - 1)]
    b_flat = n_flat * 4
    b_rows = n_ids * 16 + n_heads * D * 4
    for name, fn, k, nbytes in (
            ("grad_sqnorm_flat", lambda i: ops.grad_sqnorm_flat(flats[i], partials, 0), k_flat, b_flat),
            ("grad_sqnorm_rows", lambda i: ops.grad_sqnorm_rows(rows[i], sg.sorted_ids, opt.table.shape[0], partials, p_flat), k_rows, b_rows),
            ("grad_clip_coef", lambda i: ops.grad_clip_coef(partials, p_flat + p_rows, 1.0, 1.0, state), 1, (p_flat + p_rows) * 8)):
        hot = timed(fn, 1, args.reps)
        cold = timed(fn, k, args.reps) if k > 1 else hot
        print(f"{name:18s} {nbytes / 1e6:8.2f} MB  same buffer {hot:7.1f} us ({nbytes / hot / 1e3:7.0f} GB/s)   "
              f"rotating over {k:3d} buffers {cold:7.1f} us ({nbytes / cold / 1e3:7.0f} GB/s, {nbytes / cold / 1e3 / HBM_GBS:.1%} of 8 TB/s)")

    def trio(i):
        ops.grad_sqnorm_flat(flats[i % k_flat], partials, 0)
        ops.grad_sqnorm_rows(rows[i % k_rows], sg.sorted_ids, opt.table.shape[0], partials, p_flat)
        ops.grad_clip_coef(partials, p_flat + p_rows, 1.0, 1.0, state)
    print(f"all three launches back to back: same buffers {timed(trio, 1, args.reps):.1f} us, rotating "
          f"{timed(trio, k_flat * k_rows, args.reps):.1f} us per step")
    del flats, rows, tr, opt, model, sg
    torch.cuda.empty_cache()

    # the whole step, replayed from its hipGraph (window rows, no packing hint), with the key off and on, alternating
    def step_ms(clip):
        c = apply_run_fixups(Config(config_dict=dict(cfgd, hip_graph=True, hip_graph_required=True, clip_grad_norm=clip)))
        c["int_to_category"] = data.int_to_category
        torch.manual_seed(2020)
        m = get_model("HSTU")(c, data).to(dev)
        t = Trainer(c)
        t.setup_model(m)
        t.train_step = 3000
        m.train()
        batches = [data.train_batch(c["train_batch_size"]) for _ in range(4)]
        for i in range(12):
            t.train_step_fn(batches[i % 4])
        assert t.graph_active
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            t.train_step_fn(batches[i % 4])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps
    for rep in range(args.step_repeats):
        off, on = step_ms(None), step_ms(1.0)
        print(f"replayed step, repeat {rep}: clip_grad_norm off {off:.3f} ms, on {on:.3f} ms ({(on - off) * 1e3:+.0f} us)")


if __name__ == "__main__":
    main()
