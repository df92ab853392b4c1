"""A minimum-risk step (TrainStep.mrt_step) taken apart and timed, at 16 source sentences x 16 rows each (15 candidates of a
stochastic beam search + the gold sentence, max_length 40) on the cfg2 model of bench.py (untrained, so every draw runs 40 steps):

    draw          the candidates on the current weights (beamsearch_stochastic's search, the tokens stay on the device)
    pack + BLEU   vag_mrt_pack, vag_mbr_select against the gold rows, the expansion of source / lengths / image to 256 rows
    forced step   vag_train_step with mrt_n = 16 over the 256 rows (graph replay) + the optimiser
    mrt_step      the whole call

against a plain ``step`` on the same 256 rows (teacher-forced, graph replay, optimiser included) -- of this tree and, with
``--parent DIR`` (a built checkout of the parent commit), of the parent in a child process of the same run.

Every figure: a host clock around `reps` calls closed by a device synchronise, after a warm-up; `rounds` such windows per variant,
the variants alternating inside every round; median, min, max of the windows.

It also measures the number tests/test_gpu_mrt.py's gradient tolerance rests on: the plain NLL step, fused against the generic
per-operator path, at that test's shape (test_gpu_label_smoothing._model_case; no ranking criterion), as the largest gradient error
relative to each reference tensor's largest entry -- with ``--parent`` on the parent commit.
It fails without a GPU.

Usage (GPU box):  python tools/exp_mrt.py [--rounds 3] [--reps 5] [--parent DIR] [--out profiles/exp_mrt.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, NC, ML = 16, 15, 40


def _paths(root):
    for p in (os.path.join(root, "tests"), os.path.join(root, "vag-nmt_amd"), root):
        sys.path.insert(0, p)


def _driver(bench, torch, dev):
    from vagnmt_hip.trainer import TrainStep
    c = dict(bench.CFG2)
    c["B"] = G
    m = bench.build_model(c, dev, dropout=False)
    vw = torch.ones(c["V"], device=dev)
    vw[0] = 0
    ts = TrainStep(m, torch.nn.NLLLoss(weight=vw, reduction="none"), None, lr=4e-4, weight_decay=1e-5, clip=1.0,
                   teacher_force_ratio=1.0)
    return c, m, ts


def _windows(variants, rounds, reps, torch):
    times = {name: [] for name, _ in variants}
    for _, fn in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for r in range(rounds):
        for name, fn in (variants if r % 2 == 0 else variants[::-1]):
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps * 1e3)
    return times


def plain_only(a):
    """Child process: the plain step on the saved rows, and the NLL step's fused-against-generic gradient error."""
    import torch
    import bench
    dev = torch.device("cuda:0")
    c, m, ts = _driver(bench, torch, dev)
    src, lens, rows, im = [t.to(dev) for t in torch.load(a.rows)]
    times = _windows([("plain", lambda: ts.step(src, lens, rows, im, teacher=True))], a.rounds, a.reps, torch)
    print("EXP_MRT_CHILD " + json.dumps({"plain": times["plain"], "rel_err": nll_step_rel_err(torch)}))
    return 0


def nll_step_rel_err(torch):
    """The plain NLL step at the minimum-risk test's shape: fused step against the generic criterion path, the largest gradient error
    relative to each reference tensor's largest entry, per model kind."""
    from test_gpu_label_smoothing import _model_case, _visits
    from vagnmt_hip.trainer import TrainStep, _AutogradBackend, _FusedBackend

    class Generic(torch.nn.NLLLoss):          # recognised by nothing: log-probabilities materialised, the criterion called per step
        pass
    out = {}
    for kind in ("mm", "text"):
        m0, batch, V = _model_case(kind)
        state = {k: v.detach().clone() for k, v in m0.state_dict().items()}
        vw = torch.ones(V, device="cuda")
        vw[0] = 0
        res = []
        for cls, backend in ((Generic, _AutogradBackend), (torch.nn.NLLLoss, _FusedBackend)):
            m, _, _ = _model_case(kind)
            m.load_state_dict(state)
            ts = TrainStep(m, cls(weight=vw, reduction="none"), None, use_graph=False, pad_src=1)
            assert type(ts.backend) is backend
            m.eval()
            res.append(_visits(ts, batch, True, 1)[0][1])
        want, got = res
        out[kind] = max((got[k].double() - want[k].double()).abs().max().item() / want[k].abs().max().item()
                        for k in want if want[k].abs().max().item() > 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its plain step, in a child process")
    ap.add_argument("--plain-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--rows", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    _paths(a.root)
    import torch
    if not torch.cuda.is_available():
        sys.exit("exp_mrt: needs a GPU")
    if a.plain_only:
        return plain_only(a)
    import bench
    from vagnmt_hip import mrt
    from vagnmt_hip.sampling import Generator
    dev = torch.device("cuda:0")
    c, m, ts = _driver(bench, torch, dev)
    src, lens, tgt, im = bench.make_batch(c, 0, dev, ragged=True)
    lt = torch.tensor(lens, dtype=torch.int32, device=dev)
    gen = Generator(1)
    alpha = 5e-3
    be = ts.backend
    held = {}

    def draw():
        held["cand"] = mrt._draw(ts, src, lt, im, NC, ML, "stochastic", gen)

    def prepare():
        held["prep"] = mrt._prepare(src, lt, tgt, im, held["cand"], 1)

    def forced():
        rows, valid, cost, N, src_r, len_r, im_r = held["prep"]
        ts.model.train()
        mrt._run_groups(be, G, N, alpha, 1024, rows, valid, cost, src_r, len_r, im_r, 7)
        ts._run_optimizer()

    draw()
    prepare()
    rows, valid, cost, N, src_r, len_r, im_r = held["prep"]
    assert rows.shape[0] == G * (NC + 1) == 256
    variants = [("draw", draw), ("pack+BLEU", prepare), ("forced step", forced),
                ("mrt_step", lambda: ts.mrt_step(src, lt, tgt, im, n_candidates=NC, alpha=alpha, max_length=ML, generator=gen)),
                ("plain step", lambda: ts.step(src_r, len_r, rows, im_r, teacher=True))]
    times = _windows(variants, a.rounds, a.reps, torch)
    rel = nll_step_rel_err(torch)
    lines = ["tools/exp_mrt.py on %s: %d sentences x %d rows (%d candidates of a stochastic beam search + gold), max_length %d, "
             "forced rows (256, %d), V %d, alpha %g; ms per call, %d rounds x %d calls per window"
             % (torch.cuda.get_device_name(0), G, N, NC, ML, rows.shape[1], c["V"], alpha, a.rounds, a.reps)]
    base = statistics.median(times["plain step"])
    for name, _ in variants:
        xs = times[name]
        lines.append("  %-12s median %8.3f  min %8.3f  max %8.3f   %5.2f x plain step"
                     % (name, statistics.median(xs), min(xs), max(xs), statistics.median(xs) / base))
    lines.append("valid rows per sentence in the timed set: min %d, max %d of %d"
                 % (int(valid.view(G, N).sum(1).min()), int(valid.view(G, N).sum(1).max()), N))
    lines.append("NLL step at the gradient test's shape (H 64, V 61, B 8, Ts 9, Tt 7), fused against generic, largest gradient error / "
                 "reference max: this tree  mm %.3e  text %.3e" % (rel["mm"], rel["text"]))
    if a.parent:
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "rows.pt")
            torch.save([t.cpu() for t in (src_r, len_r, rows, im_r)], path)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--root", os.path.abspath(a.parent),
                                "--rows", path, "--rounds", str(a.rounds), "--reps", str(a.reps)], capture_output=True, text=True,
                               timeout=900)
        if r.returncode != 0:
            sys.exit("exp_mrt: the parent's run failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
        child = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("EXP_MRT_CHILD ")][-1][len("EXP_MRT_CHILD "):])
        xs = child["plain"]
        lines.append("parent commit, same run, same rows:")
        lines.append("  %-12s median %8.3f  min %8.3f  max %8.3f   (this tree's plain step: %.3f x)"
                     % ("plain step", statistics.median(xs), min(xs), max(xs), base / statistics.median(xs)))
        lines.append("  NLL step, fused against generic, largest gradient error / reference max: parent  mm %.3e  text %.3e"
                     % (child["rel_err"]["mm"], child["rel_err"]["text"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
