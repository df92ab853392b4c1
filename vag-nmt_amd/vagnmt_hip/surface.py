"""Surface table: what the target vocabulary's ids spell, for utilities that are defined on characters (chrF: vagnmt_hip.mbr,
utility="chrf"; include/vag_nmt.h: vag_surface_expand, vag_chrf_select).

    table = Surface(words)                  # words[i]: the string of target id i (the reference's index-to-word list)
    table.off (V + 1,) int32, table.chars (off[V],) int32      the table, CSR, on the device (built on the first use there)
    table.max_len                           the longest surface, in characters (host)
    table.text(tokens)                      the Python string of a token list cut at EOS (host)

The surface of id i is words[i] with ONE trailing join marker ("@@", the BPE continuation mark) stripped and all whitespace
removed, as Unicode code points (Python's ord: "ä" is one character).  The ids in `empty` (padding 0, SOS 2, EOS 3) have the
empty surface; UNK keeps its literal string.  chrF ignores whitespace, so the character row of a sentence is the concatenation
of its tokens' surfaces and BPE joins need nothing more."""
import torch

from vagnmt_hip._lib import call, lib, ptr, stream
from vagnmt_hip.search import EOS_token


class Surface:
    def __init__(self, words, join="@@", empty=(0, 2, 3)):
        words = list(words)
        if not words or not all(isinstance(w, str) for w in words):
            raise ValueError("Surface: words must be a non-empty list of strings (words[i]: the string of target id i)")
        if not isinstance(join, str):
            raise ValueError("Surface: join must be a string ('' for none), got %r" % (join,))
        self.V = len(words)
        self.join = join
        self.empty = frozenset(int(i) for i in empty)
        self.surfaces = []
        for i, w in enumerate(words):
            if i in self.empty:
                w = ""
            elif join and w.endswith(join):
                w = w[:-len(join)]
            self.surfaces.append("".join(w.split()))
        lens = [len(s) for s in self.surfaces]
        self.max_len = max(lens)
        if sum(lens) >= 1 << 31:
            raise ValueError("Surface: the table holds %d characters, the offsets are int32" % sum(lens))
        self._off = torch.zeros(self.V + 1, dtype=torch.int32)
        self._off[1:] = torch.tensor(lens, dtype=torch.int64).cumsum(0).to(torch.int32)
        # (one spare element keeps chars non-empty for a table of empty surfaces; off[V] is the count)
        self._chars = torch.tensor([ord(c) for s in self.surfaces for c in s] + [0], dtype=torch.int32)
        self._dev = {}

    def host(self):
        """(off (V + 1,), chars (off[V] + 1,)) int32 CPU tensors; the last element of chars is a spare 0."""
        return self._off, self._chars

    def on(self, device):
        """(off, chars) on `device`, copied there once."""
        key = torch.device(device)
        if key not in self._dev:
            self._dev[key] = (self._off.to(key), self._chars.to(key))
        return self._dev[key]

    @property
    def off(self):
        return self.on(torch.device("cuda", torch.cuda.current_device()))[0]

    @property
    def chars(self):
        return self.on(torch.device("cuda", torch.cuda.current_device()))[1][:-1]

    def text(self, tokens):
        """The string of a token list: the surfaces of the tokens before the first EOS, concatenated."""
        out = []
        for t in tokens:
            t = int(t)
            if t == EOS_token:
                break
            out.append(self.surfaces[t])
        return "".join(out)

    def row_chars(self, L):
        """C of the expansion of rows of L tokens: min(the kernel's limit, L * max_len), at least 1."""
        return max(1, min(int(lib().vag_chrf_max_chars()), int(L) * self.max_len))

    def expand(self, rows, C=None):
        """vag_surface_expand: rows (..., L) int64 on a GPU, ids below V -> (chars (..., C) int32, lens (...,) int32) there; lens
        holds the true character counts, chars their first min(lens, C).  One launch, nothing waits for the host."""
        shape = tuple(rows.shape[:-1])
        L = rows.shape[-1]
        C = self.row_chars(L) if C is None else int(C)
        rows = rows.contiguous()
        R = rows.numel() // L
        off, chars = self.on(rows.device)
        out = torch.empty(shape + (C,), dtype=torch.int32, device=rows.device)
        lens = torch.empty(shape, dtype=torch.int32, device=rows.device)
        call("vag_surface_expand", ptr(rows, torch.int64), R, L, ptr(off, torch.int32), ptr(chars, torch.int32), self.V,
             ptr(out, torch.int32), C, ptr(lens, torch.int32), stream())
        return out, lens
