"""Validation on the device: what the reference's loop does every ``eval_every`` steps (nmt_multimodal_beam_DE.py:418-522) -- the
dev loss, a beam-search decode of the dev set, corpus BLEU, the plateau rule on the learning rate, "best" flags and early
stopping -- with the per-batch work left on the GPU and ONE read of the device at the end.

    v = validate(ts, dev_batches, beam_size=12, max_length=80)              # ts: a TrainStep; batches of (src, lengths, tgt, im)
    v.loss, v.loss_mt, v.loss_vse      floats: the mean over the batches of TrainStep.eval_loss, as the reference reports it
    v.bleu                             CorpusBLEU(bleu, precisions, bp, ratio, translation_length, reference_length)
    v.chrf                             float or None (metrics=("loss", "bleu", "chrf"), surface=Surface(words))
    verdict = monitor.update(ts, v)    # Monitor(): Verdict(best_loss, best_bleu, lr, stop)

    with ts.averaged_weights():        # validation on the averaged weights
        v = validate(ts, dev_batches)

The metrics alone:

    stats = BleuStats(device); stats.add(hyps, refs); ...; stats.result(smooth=False)      # accumulates, no host sync in add
    corpus_bleu(hyps, refs, n_refs=None, smooth=False)                                     # one shot
    ChrfStats(device, surface) / corpus_chrf(hyps, refs, surface)

Corpus BLEU is the reference's bleu.compute_bleu: the integer statistics come from vag_corpus_bleu_stats (csrc/corpus.hip: clipped
1..4-gram matches against the MERGED counts of up to 64 references per sentence, rows of up to 512 tokens), the score is formed
from the ten totals on the host in Python floats with the reference's operations in the reference's order.  Corpus chrF is the
project's sentence-level chrF (include/vag_nmt.h: vag_chrf_select) pooled over the corpus: per order n = 1..6 the totals M_n of
the matches and H_n, R_n of the n-grams of the hypotheses and references (from the STORED character counts: a sentence beyond
the kernel's 1024 characters is cut, as everywhere); an order is effective when H_n > 0 and R_n > 0; P = the mean of M_n / H_n
over the effective orders, R likewise, F = 5 P R / (4 P + R) in float64, 0 with no effective order or P + R = 0.  Single
reference only; chrF++, METEOR and perplexity are not computed.

Limits: the dev loss needs the fused backend on one GPU (TrainStep.eval_loss); validation is not sharded over ranks."""
import math
from collections import namedtuple

import torch

from vagnmt_hip._lib import call, lib, ptr, stream
from vagnmt_hip.search import EOS_token, cut

CorpusBLEU = namedtuple("CorpusBLEU", ["bleu", "precisions", "bp", "ratio", "translation_length", "reference_length"])
Validation = namedtuple("Validation", ["loss", "loss_mt", "loss_vse", "bleu", "chrf", "n_sentences", "n_batches", "translations"])
Verdict = namedtuple("Verdict", ["best_loss", "best_bleu", "lr", "stop"])

METRICS = ("loss", "bleu", "chrf")
CHRF_ORDER = 6
_CHRF_ROWS = 1 << 20            # sentences per vag_chrf_select call (its limit: B < 2^21)


# ------------------------------------------------------------------------------------------------------------------
# the host finish
# ------------------------------------------------------------------------------------------------------------------
def bleu_from_totals(totals, smooth=False):
    """CorpusBLEU from the ten totals (m_1..m_4, T_1..T_4, translation length, reference length): bleu.py:85-116 in Python
    floats, operation for operation.  reference_length == 0 raises ValueError (bleu.py divides by zero there)."""
    t = [int(x) for x in totals]
    if len(t) != 10:
        raise ValueError("bleu_from_totals: ten totals, got %d" % len(t))
    matches, possible, tl, rl = t[0:4], t[4:8], t[8], t[9]
    if rl == 0:
        raise ValueError("corpus BLEU: the reference length is 0 (no sentence added, or only empty references)")
    precisions = [0] * 4
    for i in range(4):
        if smooth:
            precisions[i] = (matches[i] + 1.) / (possible[i] + 1.)
        elif possible[i] > 0:
            precisions[i] = float(matches[i]) / possible[i]
        else:
            precisions[i] = 0.0
    if min(precisions) > 0:
        geo_mean = math.exp(sum((1. / 4) * math.log(p) for p in precisions))
    else:
        geo_mean = 0
    ratio = float(tl) / rl
    if ratio > 1.0:
        bp = 1.
    elif ratio == 0.0:
        bp = 0.
    else:
        bp = math.exp(1 - 1. / ratio)
    return CorpusBLEU(geo_mean * bp, precisions, bp, ratio, tl, rl)


def chrf_from_totals(totals):
    """Corpus chrF (float64) from the 18 totals M_1..M_6, H_1..H_6, R_1..R_6 -- the module's text has the definition."""
    t = [int(x) for x in totals]
    if len(t) != 3 * CHRF_ORDER:
        raise ValueError("chrf_from_totals: %d totals, got %d" % (3 * CHRF_ORDER, len(t)))
    M, H, R = t[0:6], t[6:12], t[12:18]
    sp = sr = 0.0
    orders = 0
    for n in range(CHRF_ORDER):
        if H[n] > 0 and R[n] > 0:
            sp += M[n] / H[n]
            sr += M[n] / R[n]
            orders += 1
    if orders == 0:
        return 0.0
    P, Rc = sp / orders, sr / orders
    if P + Rc == 0.0:
        return 0.0
    return 5.0 * P * Rc / (4.0 * P + Rc)


# ------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------
def _is_tokens(x):
    return len(x) == 0 or not isinstance(x[0], (list, tuple))


def _pack_rows(rows):
    """Token lists -> (N, L) int64 CPU tensor the way mbr.pack packs a row: EOS appended to a list that holds none, padded with 0."""
    rows = [[int(t) for t in r] for r in rows]
    rows = [r if EOS_token in r else r + [EOS_token] for r in rows]
    out = torch.zeros(len(rows), max(len(r) for r in rows), dtype=torch.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.tensor(r, dtype=torch.int64)
    return out


def _device(device):
    device = torch.device("cuda") if device is None else torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _rows(t, what, where, device):
    """One (N, L) int64 operand on the device: a GPU tensor, or token lists."""
    if torch.is_tensor(t):
        if not t.is_cuda:
            raise ValueError("%s: %s must be a GPU tensor or token lists (there is no CPU path)" % (where, what))
        if t.dtype != torch.int64:
            raise ValueError("%s: %s must be int64, got %s" % (where, what, t.dtype))
        return t
    t = list(t)
    if not t:
        raise ValueError("%s: %s is empty" % (where, what))
    return _pack_rows(t).to(device)


def bleu_args(hyps, refs, n_refs=None, device=None, where="corpus_bleu"):
    """Host-side checks of BleuStats.add; returns (hyps (N, Lh), refs (N, R, Lr), n_refs (N,) int32 or None) on the device,
    contiguous.  hyps: a (N, Lh) int64 GPU tensor or N token lists.  refs: (N, R, Lr) or (N, Lr) int64 GPU tensor; or N token
    lists (one reference each); or refs[b] = a list of that sentence's reference token lists -- sentences may then have
    different numbers of references, which sets n_refs.  n_refs: None, an int, or N ints / an integer tensor, 1 <= n <= R.
    Nothing here reads the device."""
    dev = _device(device)
    hyps = _rows(hyps, "hyps", where, dev)
    if hyps.dim() != 2 or min(hyps.shape) < 1:
        raise ValueError("%s: hyps must be (N, Lh), got %s" % (where, tuple(hyps.shape)))
    N = hyps.shape[0]
    if torch.is_tensor(refs):
        refs = _rows(refs, "refs", where, dev)
        if refs.dim() == 2:
            refs = refs[:, None, :]
    else:
        refs = list(refs)
        if not refs:
            raise ValueError("%s: refs is empty" % where)
        if all(_is_tokens(r) for r in refs):
            refs = _pack_rows(refs)[:, None, :].to(dev)
        else:
            counts = [len(r) for r in refs]
            if min(counts) < 1:
                raise ValueError("%s: every sentence needs at least one reference" % where)
            R = max(counts)
            flat = _pack_rows([r for sent in refs for r in list(sent) + [[]] * (R - len(sent))])
            refs = flat.view(len(counts), R, -1).to(dev)
            if n_refs is None and min(counts) != R:
                n_refs = counts
    if refs.dim() != 3 or min(refs.shape) < 1 or refs.shape[0] != N:
        raise ValueError("%s: refs must be (N, R, Lr) or (N, Lr) with N = %d, got %s" % (where, N, tuple(refs.shape)))
    if refs.device != hyps.device:
        raise ValueError("%s: hyps and refs are on different devices" % where)
    R = refs.shape[1]
    if not lib().vag_corpus_bleu_supported(hyps.shape[1], R, refs.shape[2]):
        raise ValueError("%s: unsupported shape: hyps %s, refs %s (rows of up to 512 tokens, up to 64 references; include/vag_nmt.h: "
                         "vag_corpus_bleu_stats)" % (where, tuple(hyps.shape), tuple(refs.shape)))
    if n_refs is not None:
        if torch.is_tensor(n_refs):
            if n_refs.dtype.is_floating_point or tuple(n_refs.shape) != (N,):
                raise ValueError("%s: n_refs must hold N = %d integers, got %s %s" % (where, N, n_refs.dtype, tuple(n_refs.shape)))
            n_refs = n_refs.to(device=hyps.device, dtype=torch.int32)
        else:
            vals = [int(n_refs)] * N if isinstance(n_refs, int) else [int(x) for x in n_refs]
            if len(vals) != N or min(vals) < 1 or max(vals) > R:
                raise ValueError("%s: n_refs must hold N = %d counts in [1, R = %d]" % (where, N, R))
            n_refs = torch.tensor(vals, dtype=torch.int32).to(hyps.device)
        n_refs = n_refs.contiguous()
    return hyps.contiguous(), refs.contiguous(), n_refs


# ------------------------------------------------------------------------------------------------------------------
# accumulators
# ------------------------------------------------------------------------------------------------------------------
class BleuStats:
    """Corpus BLEU accumulated on the device: ``add`` enqueues one launch of vag_corpus_bleu_stats on the running totals (no host
    sync), ``result`` reads them (one copy of 80 bytes) and finishes on the host."""

    def __init__(self, device=None):
        self.device = _device(device)
        self.totals = torch.zeros(10, dtype=torch.int64, device=self.device)

    def reset(self):
        self.totals.zero_()

    def add(self, hyps, refs, n_refs=None, per_sentence=False):
        """Adds N sentences (bleu_args documents the operands).  Returns None, or with per_sentence the (N, 10) int32 tensor of
        m_1..m_4, T_1..T_4, l_h, l_r on the device."""
        hyps, refs, n_refs = bleu_args(hyps, refs, n_refs, self.device, "BleuStats.add")
        if hyps.device != self.device:
            raise ValueError("BleuStats.add: the operands are on %s, the totals on %s" % (hyps.device, self.device))
        N, Lh = hyps.shape
        _, R, Lr = refs.shape
        ps = torch.empty(N, 10, dtype=torch.int32, device=self.device) if per_sentence else None
        call("vag_corpus_bleu_stats", ptr(hyps, torch.int64), ptr(refs, torch.int64), ptr(n_refs, torch.int32), N, Lh, R, Lr,
             ptr(ps, torch.int32), ptr(self.totals, torch.int64), stream())
        return ps

    def result(self, smooth=False):
        """CorpusBLEU of everything added so far (bleu.compute_bleu's six values); ValueError while the reference length is 0."""
        return bleu_from_totals(self.totals.cpu().tolist(), smooth)


def corpus_bleu(hyps, refs, n_refs=None, smooth=False):
    """bleu.compute_bleu(refs, hyps, smooth=smooth) of one corpus: CorpusBLEU.  Operands as BleuStats.add takes them."""
    dev = next((t.device for t in (hyps, refs) if torch.is_tensor(t) and t.is_cuda), None)
    stats = BleuStats(dev)
    stats.add(hyps, refs, n_refs)
    return stats.result(smooth)


class ChrfStats:
    """Corpus chrF accumulated on the device: ``add`` expands both sides to character rows (vag_surface_expand), takes the clipped
    character n-gram matches of every sentence pair from vag_chrf_select at Nh = Nr = 1, and adds them and the n-gram totals to 18
    int64 totals with torch on the device (no host sync); ``result`` reads them once and finishes in float64.  Ids outside the
    surface table contribute no character (vag_surface_expand)."""

    def __init__(self, device=None, surface=None):
        from vagnmt_hip.surface import Surface
        if not isinstance(surface, Surface):
            raise ValueError("ChrfStats: surface must be a vagnmt_hip.surface.Surface of the target vocabulary, got %r" % (surface,))
        self.device = _device(device)
        self.surface = surface
        self.totals = torch.zeros(3 * CHRF_ORDER, dtype=torch.int64, device=self.device)
        self._n = torch.arange(CHRF_ORDER, dtype=torch.int64, device=self.device)

    def reset(self):
        self.totals.zero_()

    def _side(self, rows, what):
        rows = _rows(rows, what, "ChrfStats.add", self.device)
        if rows.dim() == 3 and rows.shape[1] == 1:
            rows = rows[:, 0]
        if rows.dim() != 2 or min(rows.shape) < 1:
            raise ValueError("ChrfStats.add: %s must be (N, L) token rows (chrF is single-reference), got %s"
                             % (what, tuple(rows.shape)))
        if rows.shape[1] > 512:
            raise ValueError("ChrfStats.add: rows of up to 512 tokens, %s has %d" % (what, rows.shape[1]))
        if rows.device != self.device:
            raise ValueError("ChrfStats.add: %s is on %s, the totals on %s" % (what, rows.device, self.device))
        return rows.contiguous()

    def add(self, hyps, refs):
        hyps, refs = self._side(hyps, "hyps"), self._side(refs, "refs")
        if hyps.shape[0] != refs.shape[0]:
            raise ValueError("ChrfStats.add: %d hypotheses, %d references" % (hyps.shape[0], refs.shape[0]))
        for lo in range(0, hyps.shape[0], _CHRF_ROWS):
            self._add(hyps[lo:lo + _CHRF_ROWS], refs[lo:lo + _CHRF_ROWS])

    def _add(self, hyps, refs):
        N, dev = hyps.shape[0], self.device
        hchars, hlens = self.surface.expand(hyps)
        rchars, rlens = self.surface.expand(refs)
        Ch, Cr = hchars.shape[1], rchars.shape[1]
        matches = torch.empty(N, CHRF_ORDER, dtype=torch.int32, device=dev)
        expected = torch.empty(N, dtype=torch.float32, device=dev)
        best = torch.empty(N, dtype=torch.int64, device=dev)
        call("vag_chrf_select", ptr(hchars, torch.int32), ptr(hlens, torch.int32), ptr(rchars, torch.int32), ptr(rlens, torch.int32),
             None, N, 1, Ch, 1, Cr, ptr(matches, torch.int32), None, ptr(expected), ptr(best, torch.int64), stream())
        # T_n of the STORED rows, l = min(max(len, 0), C), as the header defines them
        th = (hlens.to(torch.int64).clamp_(0, Ch)[:, None] - self._n[None, :]).clamp_(min=0).sum(0)
        tr = (rlens.to(torch.int64).clamp_(0, Cr)[:, None] - self._n[None, :]).clamp_(min=0).sum(0)
        self.totals += torch.cat([matches.sum(0, dtype=torch.int64), th, tr])

    def result(self):
        return chrf_from_totals(self.totals.cpu().tolist())


def corpus_chrf(hyps, refs, surface):
    """Corpus chrF of hypotheses against one reference each (the module's text has the definition): a float64 Python float."""
    dev = next((t.device for t in (hyps, refs) if torch.is_tensor(t) and t.is_cuda), None)
    stats = ChrfStats(dev, surface)
    stats.add(hyps, refs)
    return stats.result()


# ------------------------------------------------------------------------------------------------------------------
# the validation pass
# ------------------------------------------------------------------------------------------------------------------
def _check_metrics(metrics, surface, has_loss):
    metrics = (metrics,) if isinstance(metrics, str) else tuple(metrics)
    if not metrics or any(m not in METRICS for m in metrics):
        raise ValueError("validate: metrics must be chosen from %s, got %r" % (list(METRICS), metrics))
    if "loss" in metrics and not has_loss:
        raise ValueError("validate: the dev loss needs a TrainStep (its criteria and the fused step); a model or an Ensemble "
                         "validates with metrics=('bleu',)")
    if "chrf" in metrics and surface is None:
        raise ValueError("validate: metrics 'chrf' needs surface=, the target vocabulary's vagnmt_hip.surface.Surface")
    if "chrf" not in metrics and surface is not None:
        raise ValueError("validate: surface goes with the metric 'chrf' only")
    return metrics


def validate(target, batches, beam_size=12, max_length=80, metrics=("loss", "bleu"), surface=None, refs=None,
             keep_translations=False, teacher=True):
    """One validation pass (the module's text).  target: a TrainStep, a model or an Ensemble; only a TrainStep has a dev loss.
    batches yields (src, lengths, tgt, im) as ``step`` takes them (im None for a text-only model).  The references are the tgt
    rows; refs optionally yields (refs (B, R, Lr), n_refs or None) per batch for multi-reference sets (BLEU; chrF keeps tgt).
    Per batch: ``eval_loss`` added to a device accumulator, the decode with its rows kept on the device, ``BleuStats.add`` /
    ``ChrfStats.add``.  The device is read once after the last batch -- the metrics' totals and the loss sums in one copy (the decode's
    own poll of its alive counter stays).  keep_translations: the token lists of every sentence, cut at EOS, in ``translations`` (one
    more copy at the end).
    Returns Validation(loss, loss_mt, loss_vse, bleu, chrf, n_sentences, n_batches, translations); what was not asked for is None."""
    from vagnmt_hip.trainer import TrainStep
    ts = target if isinstance(target, TrainStep) else None
    decoder = ts.model if ts is not None else target
    if not (hasattr(decoder, "beamsearch_decode") and hasattr(decoder, "_decode")):
        raise ValueError("validate: target must be a TrainStep, a model or an Ensemble, got %s" % type(target).__name__)
    metrics = _check_metrics(metrics, surface, ts is not None)
    k, ml = int(beam_size), int(max_length)
    if k < 1 or ml < 1:
        raise ValueError("validate: beam_size and max_length must be at least 1, got %d, %d" % (k, ml))
    decode = "bleu" in metrics or "chrf" in metrics or keep_translations
    refs = iter(refs) if refs is not None else None
    acc = bleu = chrf = None
    rows, n_sent, n_batches = [], 0, 0
    was = [(m, m.training) for m in (decoder.models if hasattr(decoder, "models") else [decoder])]
    try:
        for m, _ in was:
            m.eval()
        for src, lengths, tgt, im in batches:
            dev = src.device
            if "loss" in metrics:
                out = torch.stack(ts.eval_loss(src, lengths, tgt, im, teacher=teacher))
                acc = out if acc is None else acc + out
            if decode:
                out = decoder._decode(src, lengths, im, k, ml, None, device_rows=True)      # (beamsearch_decode, rows kept on the device)
                if "bleu" in metrics:
                    bleu = bleu or BleuStats(dev)
                    r, nr = next(refs) if refs is not None else (tgt, None)
                    bleu.add(out, r, nr)
                if "chrf" in metrics:
                    chrf = chrf or ChrfStats(dev, surface)
                    chrf.add(out, tgt)
                if keep_translations:
                    rows.append(out)
            n_sent += int(src.shape[0])
            n_batches += 1
    finally:
        for m, t in was:
            m.train(t)
    if n_batches == 0:
        raise ValueError("validate: no batches")
    # the one read: the int64 totals of the metrics, then the three float sums, as bytes of one buffer
    parts = [t for t in (bleu.totals if bleu is not None else None, chrf.totals if chrf is not None else None, acc) if t is not None]
    loss, got_bleu, got_chrf, at = [None, None, None], None, None, 0
    if parts:
        host = torch.cat([t.contiguous().view(torch.uint8) for t in parts]).cpu()
        if bleu is not None:
            got_bleu, at = bleu_from_totals(host[at:at + 80].view(torch.int64).tolist()), at + 80
        if chrf is not None:
            got_chrf, at = chrf_from_totals(host[at:at + 8 * 3 * CHRF_ORDER].view(torch.int64).tolist()), at + 8 * 3 * CHRF_ORDER
        if acc is not None:
            loss = [x / n_batches for x in host[at:at + 12].view(torch.float32).tolist()]
    translations = None
    if keep_translations:
        translations = [[int(t) for t in row] for row in cut(torch.cat(rows).cpu().tolist())]       # (every batch's rows are (B, max_length))
    return Validation(loss[0], loss[1], loss[2], got_bleu, got_chrf, n_sent, n_batches, translations)


# ------------------------------------------------------------------------------------------------------------------
# the loop's bookkeeping
# ------------------------------------------------------------------------------------------------------------------
class Monitor:
    """What the reference's loop keeps between validations (nmt_multimodal_beam_DE.py:469-522), on the host:
      * the plateau rule on loss_mt: torch.optim.lr_scheduler.ReduceLROnPlateau(mode="min", factor=lr_factor,
        patience=lr_patience) with its defaults (relative threshold 1e-4, cooldown 0, eps 1e-8), stepped through ``ts.set_lr``;
      * the best dev loss and the best BLEU so far -- ``best_loss`` / ``best_bleu`` of the verdict say "save that checkpoint now";
      * early stopping: ``patience`` validations without a better BLEU set ``stop``.
    ``state_dict()`` / ``load_state_dict()`` carry the counters over a resume."""
    THRESHOLD, EPS = 1e-4, 1e-8

    def __init__(self, patience=10, lr_factor=0.2, lr_patience=10, min_lr=0.0):
        if int(patience) < 1 or int(lr_patience) < 0:
            raise ValueError("Monitor: patience must be at least 1 and lr_patience at least 0, got %r, %r" % (patience, lr_patience))
        if not 0.0 < float(lr_factor) < 1.0:
            raise ValueError("Monitor: lr_factor must lie inside (0, 1), got %r" % (lr_factor,))
        if float(min_lr) < 0.0:
            raise ValueError("Monitor: min_lr must not be negative, got %r" % (min_lr,))
        self.patience, self.lr_factor, self.lr_patience, self.min_lr = int(patience), float(lr_factor), int(lr_patience), float(min_lr)
        self.plateau_best, self.num_bad = float("inf"), 0          # the scheduler's `best` and `num_bad_epochs`
        self.best_loss, self.best_bleu = float("inf"), -1.0
        self.patience_left = self.patience
        self.n_updates = 0

    def _plateau(self, metric, lr):
        """One ReduceLROnPlateau.step(metric) at rate lr; returns the new rate."""
        if metric < self.plateau_best * (1.0 - self.THRESHOLD):
            self.plateau_best, self.num_bad = metric, 0
        else:
            self.num_bad += 1
        if self.num_bad > self.lr_patience:
            new = max(lr * self.lr_factor, self.min_lr)
            if lr - new > self.EPS:
                lr = new
            self.num_bad = 0
        return lr

    def update(self, ts, validation):
        """One validation's consequences.  ts: the TrainStep (its ``lr`` is read, ``set_lr`` called), or None to keep the rate out of
        it.  validation: a Validation; a missing loss_mt skips the plateau rule and the loss flag, a missing bleu the BLEU flag and
        the patience count."""
        self.n_updates += 1
        best_loss = best_bleu = False
        lr = float(ts.lr) if ts is not None else None
        loss = validation.loss_mt
        if loss is not None:
            loss = float(loss)
            if ts is not None:
                lr = self._plateau(loss, lr)
                ts.set_lr(lr)
            if loss < self.best_loss:
                self.best_loss, best_loss = loss, True
        if validation.bleu is not None:
            b = float(validation.bleu.bleu if hasattr(validation.bleu, "bleu") else validation.bleu)
            if b > self.best_bleu:
                self.best_bleu, best_bleu = b, True
                self.patience_left = self.patience
            else:
                self.patience_left -= 1
        return Verdict(best_loss, best_bleu, lr, self.patience_left <= 0)

    _STATE = ("patience", "lr_factor", "lr_patience", "min_lr", "plateau_best", "num_bad", "best_loss", "best_bleu", "patience_left",
              "n_updates")

    def state_dict(self):
        return {k: getattr(self, k) for k in self._STATE}

    def load_state_dict(self, state):
        missing = [k for k in self._STATE if k not in state]
        if missing:
            raise ValueError("Monitor.load_state_dict: missing %s" % missing)
        for k in self._STATE:
            setattr(self, k, type(getattr(self, k))(state[k]))
