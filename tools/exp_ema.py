"""Cost of the averaged weights at BASELINE configs[1] size (B=64, Ts=Tt=40, H=512, V=9391): the whole optimiser step (TrainStep.step,
graph replay, train mode) with ema_decay = 0 and ema_decay = 0.999 from this build and, with --parent-lib, with a library built from
the parent commit (which has no averaged weights: ema_decay = 0 only) -- all in one process, two rounds over the configurations.
Warm-up, then timed windows of back-to-back replays between two events; the median window is reported.

    git worktree add ../parent HEAD~1 && make -C ../parent/vag-nmt_amd/csrc -j8
    python tools/exp_ema.py --parent-lib ../parent/vag-nmt_amd/lib/libvagnmt.so [--windows 7] [--iters 50] >> profiles/exp_ema.txt

The ema_decay = 0 step is meant to be the parent's code (adam_kernel<false>, the old entry point): a difference between those two
rows beyond the windows' own spread needs an explanation before it is merged."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vag-nmt_amd")]

import torch  # noqa: E402

from exp_label_smoothing import windows  # noqa: E402

NEW_SYMBOLS = ("vag_clip_adam_flat_ema", "vag_swap_flat")


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
    a = ap.parse_args()
    import bench
    from machine_translation_vision.losses import PairwiseRankingLoss
    from vagnmt_hip import _lib
    from vagnmt_hip.trainer import TrainStep
    c = bench.CFG2
    dev = torch.device("cuda", 0)
    print("# %s, torch %s; configs[1]: %s" % (torch.cuda.get_device_name(0), torch.__version__, {k: c[k] for k in ("B", "Ts", "Tt", "H", "V")}))
    vw = torch.ones(c["V"], device=dev)
    vw[0] = 0
    src, lens, tgt, im = bench.make_batch(c, 0, dev)
    lt = torch.tensor(lens, dtype=torch.int32, device=dev)
    this = _lib.lib()
    configs = [("this build", this, 0.0), ("this build", this, 0.999)]
    if a.parent_lib:
        configs.insert(0, ("parent    ", load_parent(a.parent_lib), 0.0))
    medians = {}
    for rnd in range(a.rounds):
        for what, L, decay in configs:
            _lib._lib = L                        # every call of the driver below goes to this library
            try:
                m = bench.build_model(c, dev, dropout=True)
                ts = TrainStep(m, torch.nn.NLLLoss(weight=vw, reduction="none"), PairwiseRankingLoss(margin=0.1), lr=4e-4,
                               weight_decay=1e-5, clip=1.0, teacher_force_ratio=1.0, ema_decay=decay)
                w = windows(lambda: ts.step(src, lt, tgt, im, teacher=True), a.windows, a.iters)
                ts.check()
                n = ts.fp.n
                del ts, m
            finally:
                _lib._lib = this
            med = statistics.median(w)
            medians.setdefault((what, decay), []).append(med)
            print("round %d  step  %s ema_decay=%-5g  median %.4f ms  spread %.4f ms  (windows %s)"
                  % (rnd + 1, what, decay, med, max(w) - min(w), " ".join("%.4f" % x for x in w)))
    base = statistics.mean(medians[("this build", 0.0)])
    print("# %d parameters; means of the rounds' medians:" % n)
    for (what, decay), v in medians.items():
        print("#   %s ema_decay=%-5g  %.4f ms  (%+.4f ms, %+.2f %% against this build's ema_decay=0)"
              % (what, decay, statistics.mean(v), statistics.mean(v) - base, 100.0 * (statistics.mean(v) - base) / base))


if __name__ == "__main__":
    main()
