"""Cost of R-Drop at BASELINE configs[1] dims (Ts=Tt=40, H=512, V=9391), graph mode, train mode, 64 rows:

  * TrainStep.rdrop_step on 32 sentences (64 rows: every sentence twice) against TrainStep.step on the SAME 64 rows from this build
    -- the difference is the regulariser's own cost: the duplication of the batch on the device, one extra read of the 64 x Tt x V
    logits in the forward (the pair kernel), the d(logits) pass of rdrop.hip in place of the plain one, the loss reduction as a
    launch of its own, and the twin flag of the ranking loss;
  * with --parent-lib, TrainStep.step on those rows with a library built from the parent commit -- all in one process, alternating
    over --rounds rounds, in alternating order.  The plain step of this build is meant to be the parent's code: a difference between those two rows
    beyond the windows' own spread needs an explanation before it is merged.

By the bytes the expectation is: forward + one read of the logits (64 x 40 x 9392 x 4 B = 96 MB), backward the traffic of the pass
it replaces.  Warm-up, then timed windows of back-to-back calls between two events; the median window is reported, with the
windows' spread.

    git worktree add ../parent HEAD~1 && make -C ../parent/vag-nmt_amd/csrc -j8
    python tools/exp_rdrop.py --parent-lib ../parent/vag-nmt_amd/lib/libvagnmt.so [--windows 7] [--iters 50] --out profiles/exp_rdrop.txt"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vag-nmt_amd")]

import torch  # noqa: E402

from exp_label_smoothing import windows  # noqa: E402

NEW_SYMBOLS = ("vag_rdrop_head_ce_seq_fwd", "vag_rdrop_head_ce_seq_bwd", "vag_step_rdrop_check", "vag_train_step_rdrop")
ALPHA = 5.0


def load_parent(path):
    """The parent's library as a second, independent CDLL with every prototype it can have."""
    from vagnmt_hip import _lib
    L = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.PROTOS.items():
        if name in NEW_SYMBOLS:
            continue
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    import bench
    from machine_translation_vision.losses import PairwiseRankingLoss
    from vagnmt_hip import _lib, rdrop
    from vagnmt_hip.trainer import TrainStep
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    c = bench.CFG2
    dev = torch.device("cuda", 0)
    vw = torch.ones(c["V"], device=dev)
    vw[0] = 0
    src, lens, tgt, im = bench.make_batch(c, 0, dev)
    n = c["B"] // 2
    lt = torch.tensor(lens, dtype=torch.int32, device=dev)
    half = (src[:n].contiguous(), lt[:n].contiguous(), tgt[:n].contiguous(), im[:n].contiguous())      # 32 sentences
    rows = tuple(rdrop.twins(t) for t in half)                                                          # the same, as 64 rows
    say("# %s, torch %s; configs[1] dims %s; %d sentences = %d rows; alpha %.0f; %d windows of %d calls"
        % (torch.cuda.get_device_name(0), torch.__version__, {k: c[k] for k in ("Ts", "Tt", "H", "V")}, n, 2 * n, ALPHA, a.windows,
           a.iters))
    this = _lib.lib()
    configs = [("this build", this, "step"), ("this build", this, "rdrop_step")]
    if a.parent_lib:
        configs.insert(0, ("parent    ", load_parent(a.parent_lib), "step"))
    medians = {}
    for rnd in range(a.rounds):
        for what, L, call in (configs if rnd % 2 == 0 else configs[::-1]):      # (alternating order: what runs first runs coolest)
            _lib._lib = L                        # every call of the driver below goes to this library
            try:
                m = bench.build_model(c, dev, dropout=True)
                ts = TrainStep(m, torch.nn.NLLLoss(weight=vw, reduction="none"), PairwiseRankingLoss(margin=0.1), lr=4e-4,
                               weight_decay=1e-5, clip=1.0, teacher_force_ratio=1.0)
                if call == "step":
                    w = windows(lambda: ts.step(*rows, teacher=True), a.windows, a.iters)
                else:
                    w = windows(lambda: ts.rdrop_step(*half, alpha=ALPHA), a.windows, a.iters)
                ts.check()
                del ts, m
            finally:
                _lib._lib = this
            med = statistics.median(w)
            medians.setdefault((what, call), []).append(med)
            say("round %d  %s %-10s  median %.4f ms  spread %.4f ms  (windows %s)"
                % (rnd + 1, what, call, med, max(w) - min(w), " ".join("%.4f" % x for x in w)))
    base = statistics.mean(medians[("this build", "step")])
    say("# means of the rounds' medians:")
    for (what, call), v in medians.items():
        say("#   %s %-10s  %.4f ms  (%+.4f ms, %+.2f %% against this build's step on the same 64 rows)"
            % (what, call, statistics.mean(v), statistics.mean(v) - base, 100.0 * (statistics.mean(v) - base) / base))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
