"""The launch trace of the five expansion searches (vagnmt_hip.search: beam, beam_diverse, beam_required, beam_stochastic,
beam_penalised), pinned to tests/golden/search_launches.json: the searches are one host driver, and a change there must not move,
drop or re-order a launch, change an argument, poll the alive counter at another point or lose an entry buffer by accident.

No device: the members are stubs on CPU tensors, and search.call / ptr / stream / _capture and ops.head_logits_parts_count are
replaced.  A recorded launch is the entry name and its arguments -- a scalar by value, a pointer by the name of the entry buffer
or stub tensor it points at (``key+bytes`` inside one; ``new:dtype[shape]`` for a tensor the search allocated for itself), a
host array as the list of its elements.  A member's step is recorded the same way, so the trace also pins which words and
states every step is given.  _capture runs the body once into a list of its own; ``replay()`` appends ``replay:<name>`` and
executes the recorded launches' effects.  The one effect the searches look at is the alive counter, which the stub sets after
every expansion: never zero, or zero from step 3 on.  The library itself is loaded for the scratch-size queries only.

The golden file was written by this module's __main__ against the search.py of the commit before the driver existed:
    python tests/test_search_driver_host.py --pkg <checkout>/vag-nmt_amd --out tests/golden/search_launches.json"""
import ctypes as C
import json
import os
import sys

import pytest
import torch

B, K, V, MAX_LEN, H, TP, TS, LD = 2, 4, 11, 10, 6, 8, 5, 12
SCRIPTS = ("never", "from3")


class StubMember:
    """What search.Member offers a search, on fixed CPU tensors (one set for step 0's B rows, one for the B k rows after it)."""

    def __init__(self, rec, m, graphed):
        self.rec, self.m = rec, m
        self.H, self.V, self.Ts = H + m, V, TS
        self.mask = rec.name("m%d.mask" % m, torch.ones(B, TP))
        self.alpha = rec.name("m%d.alpha" % m, torch.zeros(B * K, TP))
        self.h = rec.name("m%d.h" % m, torch.zeros(B * K, self.H)) if graphed else None
        self.hp, self.emb = None, torch.zeros(V, 3)
        self.out = {n: (rec.name("m%d.h2%s" % (m, tag), torch.zeros(n, self.H)),
                        rec.name("m%d.logp%s" % (m, tag), torch.zeros(n, LD + m)))
                    for n, tag in ((B, "_0"), (B * K, ""))}
        self.logits = rec.name("m%d.logits" % m, torch.zeros(B * K, LD))
        self.parts = rec.name("m%d.parts" % m, torch.zeros(3, B * K, 2))

    def step(self, tok, h, rows_per_src):
        self.rec.launch("member%d.step" % self.m, self.rec.ref(tok), self.rec.ref(h), rows_per_src)
        return self.out[tok.shape[0]]

    def step_logits(self, tok, h, rows_per_src, nparts):
        self.rec.launch("member%d.step_logits" % self.m, self.rec.ref(tok), self.rec.ref(h), rows_per_src, nparts)
        return self.out[B * K][0], self.logits, self.parts


class StubConstraints:
    def __init__(self, rec):
        self.t = [rec.name("c.prefix", torch.zeros(B, 2, dtype=torch.int64)), rec.name("c.phrases", torch.zeros(3, 8, dtype=torch.int64)),
                  rec.name("c.phrase_sent", torch.zeros(3, dtype=torch.int32))]

    def args(self):
        return (self.t[0].data_ptr(), 2, self.t[1].data_ptr(), self.t[2].data_ptr(), 3, 2)


class Graph:
    def __init__(self, rec, name, launches):
        self.rec, self.name, self.launches = rec, name, launches

    def replay(self):
        self.rec.trace.append("replay:" + self.name)
        for text, effect in self.launches:
            effect()


class Recorder:
    """The replacements of search.call / ptr / stream / _capture / search_buffer and the trace they write."""

    def __init__(self, search):
        self.search = search
        self.named = {}                 # name -> tensor: the stub tensors and, through search_buffer, the search buffer's parts
        self.entry = None               # the entry dict of a graph-mode search
        self.fresh = {}                 # address -> tensor handed to ptr() that has no name
        self.trace, self.into = [], None
        self.script, self.expansions = "never", 0
        self._buffer = search.search_buffer

    def name(self, name, t):
        self.named[name] = t
        return t

    def begin(self, script, entry):
        self.trace, self.script, self.expansions, self.entry = [], script, 0, entry

    # ---- naming
    def _tensors(self):
        for d in (self.entry or {}), self.named:
            for key in sorted(d):
                if isinstance(d[key], torch.Tensor):
                    yield key, d[key]

    def resolve(self, addr):
        """(name, tensor or None) of an address: an exact match first, then the smallest named tensor that contains it."""
        inside = None
        for key, t in self._tensors():
            a, n = t.data_ptr(), t.numel() * t.element_size()
            if a == addr and key != "flat":
                return key, t
            if a <= addr < a + n and (inside is None or n < inside[2]):
                inside = (key, addr - a, n)
        if inside:
            return "%s+%d" % inside[:2], None
        t = self.fresh.get(addr)
        if t is not None:
            return "new:%s%s" % (str(t.dtype).replace("torch.", ""), list(t.shape)), t
        return None, None

    def ref(self, t):
        if t is None:
            return None
        self.fresh[t.data_ptr()] = t
        return self.resolve(t.data_ptr())[0]

    def ptr(self, t, dtype=torch.float32):
        if t is None:
            return None
        assert t.dtype == dtype and t.is_contiguous(), (t.dtype, dtype)
        self.fresh[t.data_ptr()] = t
        return t.data_ptr()

    def stream(self):
        return "stream"

    def search_buffer(self, *a, **kw):
        buf = self._buffer(*a, **kw)
        for key, t in buf.items():
            self.named[key] = t
        return buf

    def _arg(self, a):
        if isinstance(a, C.Array):
            if a._type_ is C.c_void_p:
                return [self.resolve(x)[0] if x else None for x in a]
            return [int(x) for x in a]
        if isinstance(a, bool) or a is None or isinstance(a, str):
            return a
        if isinstance(a, int):
            n = self.resolve(a)[0] if a > (1 << 20) else None
            return n if n is not None else a
        if isinstance(a, float):
            return round(a, 6)
        raise TypeError("unexpected launch argument %r" % (a,))

    # ---- launches
    def launch(self, name, *args):
        text = "%s(%s)" % (name, ", ".join(json.dumps(a) for a in args))
        (self.trace if self.into is None else self.into).append(text)
        return text

    def call(self, name, *args):
        shown = [self._arg(a) for a in args]
        text = self.launch(name, *shown)
        # the tensors behind the pointer arguments, by the name they were recorded under
        tensors = [(s, self.resolve(a)[1]) for a, s in zip(args, shown) if isinstance(a, int) and isinstance(s, str)]
        effect = lambda: self._effect(name, tensors)
        if self.into is None:
            effect()
        else:
            self.into[-1] = (text, effect)

    def _effect(self, name, tensors):
        if "_step" in name and name.startswith("vag_beam_"):          # an expansion: the scripted alive counter
            step, self.expansions = self.expansions, self.expansions + 1
            n_alive = [t for s, t in tensors if s == "n_alive"]
            assert len(n_alive) == 1, tensors
            n_alive[0].fill_(0 if self.script == "from3" and step >= 3 else 1)
        if name.startswith("vag_beam_finish"):                        # valid outputs: slots in range, words, scores
            for s, t in tensors:
                if not s.startswith("new:"):
                    continue
                if t.dtype == torch.int64 and t.dim() == 2:
                    t.copy_(torch.arange(t.shape[1]).expand_as(t))
                elif t.dtype == torch.int64:
                    t.fill_(4)
                    t[..., -1] = 3
                else:
                    t.zero_()
        if name == "vag_sample_noise":
            tensors[-1][1].zero_()

    def capture(self, entry, pool, body, name="graph"):
        self.into = []
        try:
            body()
        finally:
            launches, self.into = self.into, None
        self.trace.append({"capture:" + name: [x if isinstance(x, str) else x[0] for x in launches]})
        entry[name] = Graph(self, name, [x for x in launches if not isinstance(x, str)])


def cases():
    """(case name, search function name, M, graphed, keyword options)."""
    out = []
    for graphed in (False, True):
        for M in (1, 2):
            tag = "%s_M%d" % ("graph" if graphed else "eager", M)
            plain = [("plain", {}), ("nbest", dict(n_best=3)), ("align", dict(n_best=2, align=True)), ("constrain", dict(constrain=True))]
            if M == 1:
                plain.append(("raw_logits", dict(raw_logits=True)))
            for name, kw in plain:
                out.append(("beam_%s_%s" % (name, tag), "beam", M, graphed, kw))
            out.append(("diverse_G2_%s" % tag, "beam_diverse", M, graphed, dict(groups=2, strength=0.5)))
            for con in (False, True):
                c = "_constrain" if con else ""
                out.append(("required%s_%s" % (c, tag), "beam_required", M, graphed, dict(constrain=con)))
                out.append(("stochastic%s_%s" % (c, tag), "beam_stochastic", M, graphed, dict(constrain=con)))
                for beta in (0.0, 0.25):
                    for stepwise in (0, 1):
                        out.append(("penalised_beta%g_sw%d%s_%s" % (beta, stepwise, c, tag), "beam_penalised", M, graphed,
                                    dict(beta=beta, stepwise=stepwise, constrain=con)))
    return out


def run_case(search, ops, fn, M, graphed, kw):
    """One case under both scripts (graph mode: the second call re-uses the first one's entry) -> {script: result}."""
    saved = (search.call, search.ptr, search.stream, search._capture, search.search_buffer, ops.head_logits_parts_count)
    rec = Recorder(search)
    search.call, search.ptr, search.stream, search._capture, search.search_buffer = (rec.call, rec.ptr, rec.stream, rec.capture,
                                                                                     rec.search_buffer)
    ops.head_logits_parts_count = lambda hp, rows, E, V_: 3
    try:
        members = [StubMember(rec, m, graphed) for m in range(M)]
        h0s = [rec.name("m%d.h0" % m, torch.zeros(B, H + m)) for m in range(M)]
        kw = dict(kw)
        if kw.get("constrain") is True:
            kw["constrain"] = StubConstraints(rec)
        elif "constrain" in kw:
            kw["constrain"] = None
        entry = {"graph": None} if graphed else None
        mode = dict(entry=entry, pool=lambda: None)
        results = {}
        for script in SCRIPTS:
            rec.begin(script, entry)
            if fn == "beam":
                r = search.beam(members, h0s, K, MAX_LEN, flags=1, **mode, **kw)
            elif fn == "beam_diverse":
                r = search.beam_diverse(members, h0s, K, kw["groups"], kw["strength"], MAX_LEN, flags=2, n_best=3, **mode)
            elif fn == "beam_required":
                r = search.beam_required(members, h0s, K, MAX_LEN, torch.zeros(B, 16, 8, dtype=torch.int64), flags=1, n_best=2, **mode,
                                         **kw)
            elif fn == "beam_stochastic":
                r = search.beam_stochastic(members, h0s, K, MAX_LEN, rec.name("arg.rng", torch.zeros(2, dtype=torch.int64)), flags=3,
                                           **mode, **kw)
            else:
                tab = [1.0 + 0.5 * i for i in range(MAX_LEN + 1)]
                r = search.beam_penalised(members, h0s, K, MAX_LEN, tab, tab[::-1], kw["beta"], kw["stepwise"], flags=0, n_best=3,
                                          **mode, constrain=kw["constrain"])
            results[script] = {"trace": rec.trace, "steps": r[2], "result_len": len(r[0]),
                               "keys": sorted(entry) if graphed else None}
        return results
    finally:
        (search.call, search.ptr, search.stream, search._capture, search.search_buffer, ops.head_logits_parts_count) = saved


def all_traces(search, ops):
    return {name: run_case(search, ops, fn, M, graphed, kw) for name, fn, M, graphed, kw in cases()}


def intern(traces):
    """The golden file's form: every distinct launch text once, the traces as indices into that table."""
    table, index = [], {}

    def code(x):
        if isinstance(x, dict):
            return {k: [code(y) for y in v] for k, v in x.items()}
        if x not in index:
            index[x] = len(table)
            table.append(x)
        return index[x]

    out = {name: {script: dict(r, trace=[code(x) for x in r["trace"]]) for script, r in case.items()} for name, case in traces.items()}
    return {"shapes": dict(B=B, k=K, V=V, max_length=MAX_LEN), "launches": table, "cases": out}


def expand(golden):
    table = golden["launches"]

    def text(x):
        return {k: [text(y) for y in v] for k, v in x.items()} if isinstance(x, dict) else table[x]

    return {name: {script: dict(r, trace=[text(x) for x in r["trace"]]) for script, r in case.items()}
            for name, case in golden["cases"].items()}


@pytest.fixture(scope="module")
def golden():
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "search_launches.json")) as f:
        return expand(json.load(f))


CASES = cases()


def test_the_golden_file_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(c[0] for c in CASES)
    for case in golden.values():
        assert sorted(case) == sorted(SCRIPTS)


@pytest.mark.parametrize("name,fn,M,graphed,kw", CASES, ids=[c[0] for c in CASES])
def test_search_enqueues_the_recorded_launches(golden, name, fn, M, graphed, kw):
    from vagnmt_hip import ops, search
    got = json.loads(json.dumps(run_case(search, ops, fn, M, graphed, kw)))
    want = golden[name]
    for script in SCRIPTS:
        g, w = got[script], want[script]
        assert g["steps"] == w["steps"], (script, g["steps"], w["steps"])
        assert g["keys"] == w["keys"], script
        assert g["result_len"] == w["result_len"], script
        for i, (a, b) in enumerate(zip(g["trace"], w["trace"])):
            assert a == b, "%s, launch %d:\n got  %s\n want %s" % (script, i, a, b)
        assert len(g["trace"]) == len(w["trace"]), script
    # the scripts do what they say: every step ran, or the search stopped at the first poll after step 3
    assert want["never"]["steps"] == MAX_LEN
    assert want["from3"]["steps"] == (9 if graphed else 8)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", required=True, help="the vag-nmt_amd directory whose vagnmt_hip.search is traced")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    from vagnmt_hip import ops, search
    assert os.path.abspath(search.__file__).startswith(os.path.abspath(a.pkg)), search.__file__
    g = intern(json.loads(json.dumps(all_traces(search, ops))))
    with open(a.out, "w") as f:
        json.dump(g, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases, %d distinct launches -> %s" % (len(g["cases"]), len(g["launches"]), a.out))
