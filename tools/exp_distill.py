"""Cost of word-level distillation at BASELINE configs[1] size (B=64, Ts=Tt=40, H=512, V=9391), graph mode, train mode:

  * the whole optimiser step: TrainStep.distill_step with PRECOMPUTED soft targets (top_k = 8) against TrainStep.step on the same
    batch from this build and, with --parent-lib, against TrainStep.step with a library built from the parent commit -- all in one
    process, alternating over --rounds rounds.  By its launches a distillation step is the plain step plus two small launches per
    pass of the head (K + 1 logits of a row each);
  * the teacher pass, separately: distill.teacher_targets for a teacher of M = 1 and of M = 3 members (one teacher-forced forward
    per member, then one vag_kd_targets launch).

Warm-up, then timed windows of back-to-back calls between two events; the median window is reported, with the windows' spread.

    git worktree add ../parent HEAD~1 && make -C ../parent/vag-nmt_amd/csrc -j8
    python tools/exp_distill.py --parent-lib ../parent/vag-nmt_amd/lib/libvagnmt.so [--windows 7] [--iters 50] --out profiles/exp_distill.txt

The plain step of this build is meant to be the parent's code: a difference between those two rows beyond the windows' own spread
needs an explanation before it is merged."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vag-nmt_amd")]

import torch  # noqa: E402

from exp_label_smoothing import windows  # noqa: E402

NEW_SYMBOLS = ("vag_kd_targets", "vag_kd_head_ce_seq_fwd", "vag_kd_head_ce_seq_bwd", "vag_step_kd_check", "vag_train_step_kd")
TOP_K, KD_LAMBDA = 8, 0.5


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
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    import bench
    from machine_translation_vision.losses import PairwiseRankingLoss
    from vagnmt_hip import _lib, distill
    from vagnmt_hip.ensemble import Ensemble
    from vagnmt_hip.trainer import TrainStep
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    c = bench.CFG2
    dev = torch.device("cuda", 0)
    say("# %s, torch %s; configs[1]: %s; top_k %d, kd_lambda %.1f; %d windows of %d calls"
        % (torch.cuda.get_device_name(0), torch.__version__, {k: c[k] for k in ("B", "Ts", "Tt", "H", "V")}, TOP_K, KD_LAMBDA,
           a.windows, a.iters))
    vw = torch.ones(c["V"], device=dev)
    vw[0] = 0
    src, lens, tgt, im = bench.make_batch(c, 0, dev)
    lt = torch.tensor(lens, dtype=torch.int32, device=dev)
    this = _lib.lib()
    # the teacher pass, and the targets the timed distillation steps read
    teachers = [bench.build_model(c, dev, dropout=False) for _ in range(3)]
    soft = distill.teacher_targets(teachers[0], src, lt, tgt, im, top_k=TOP_K, vocab_size=c["V"])
    for M in (1, 3):
        teacher = teachers[0] if M == 1 else Ensemble(teachers[:M])
        w = windows(lambda: distill.teacher_targets(teacher, src, lt, tgt, im, top_k=TOP_K), a.windows, max(5, a.iters // 5), warmup=5)
        say("teacher pass  M=%d  teacher_targets (eager)  median %.4f ms  spread %.4f ms  (windows %s)"
            % (M, statistics.median(w), max(w) - min(w), " ".join("%.4f" % x for x in w)))
    del teachers
    configs = [("this build", this, "step"), ("this build", this, "distill_step")]
    if a.parent_lib:
        configs.insert(0, ("parent    ", load_parent(a.parent_lib), "step"))
    medians = {}
    for rnd in range(a.rounds):
        for what, L, call in configs:
            _lib._lib = L                        # every call of the driver below goes to this library
            try:
                m = bench.build_model(c, dev, dropout=True)
                ts = TrainStep(m, torch.nn.NLLLoss(weight=vw, reduction="none"), PairwiseRankingLoss(margin=0.1), lr=4e-4,
                               weight_decay=1e-5, clip=1.0, teacher_force_ratio=1.0)
                if call == "step":
                    w = windows(lambda: ts.step(src, lt, tgt, im, teacher=True), a.windows, a.iters)
                else:
                    w = windows(lambda: ts.distill_step(src, lt, tgt, im, soft=soft, kd_lambda=KD_LAMBDA), a.windows, a.iters)
                ts.check()
                del ts, m
            finally:
                _lib._lib = this
            med = statistics.median(w)
            medians.setdefault((what, call), []).append(med)
            say("round %d  %s %-12s  median %.4f ms  spread %.4f ms  (windows %s)"
                % (rnd + 1, what, call, med, max(w) - min(w), " ".join("%.4f" % x for x in w)))
    base = statistics.mean(medians[("this build", "step")])
    say("# means of the rounds' medians:")
    for (what, call), v in medians.items():
        say("#   %s %-12s  %.4f ms  (%+.4f ms, %+.2f %% against this build's step)"
            % (what, call, statistics.mean(v), statistics.mean(v) - base, 100.0 * (statistics.mean(v) - base) / base))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
