"""Regular expressions over the CTC lattice: the compiler from an expression to a deterministic automaton, the
host check of an automaton's tables, and the operators of the sixth C header, include/dtlr_pattern.h, over the launch seam of
dtlr_amd/_lib.py (`_lib.launch` / `_lib.query` name each symbol once, `@_lib.op` scopes a call to the device of its first tensor).
dtlr_amd/ops.py serves these functions under its own name too (ops.pattern_decode, ops.pattern_search, ...).

The compiler is written out here: a recursive-descent parser, Thompson's construction, the subset construction, a minimisation by
partition refinement, dead states trimmed.  Python's `re` is asked which charset characters `\\d`, `\\w` and `\\s` hold, never to match.

Dialect: literals and `\\`-escapes of metacharacters; `.`; classes `[a-z0-9_]` and negated classes `[^...]`; `\\d`, `\\w`, `\\s`, also inside
classes; groups `( )` and `(?: )`, both non-capturing; `|`; `*`, `+`, `?`, `{m}`, `{m,}`, `{m,n}` with n <= 64.  No anchors, back-references,
look-around or flags: an expression always stands for whole strings (decode) or whole hits (search).  Only the single-character entries
of the charset can be matched; `.` and negated classes range over exactly those."""
from __future__ import annotations

import dataclasses
import math
import re as _re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

PATTERN_WORKSPACE_LIMIT = 1 << 30           # bytes of workspace one launch may take: pattern_decode / pattern_search chunk under it
MAX_STATES = 4096
MAX_ARCS = 1 << 20
MAX_REPEAT = 64
MAX_HITS = 16
MAX_V = 15360
_GRID = 2048                                # workgroups of one launch at the most
_PATTERN_FIELDS = ("arc_src", "arc_chan", "dst_start", "accept")
_META = set("\\.[]()|*+?{}^$")


@dataclasses.dataclass
class Automaton:
    """A deterministic automaton over emission channels (channel = label + 1; 0, the blank, never labels an arc).  State 0 is the
    start.  The arcs are sorted by (dst, src, chan) and that order is the arc id; dst_start [n_states + 1] is the CSR index of the
    arcs INTO every state.  Every state is reachable and reaches an accepting state."""
    n_states: int
    arc_src: np.ndarray
    arc_chan: np.ndarray
    arc_dst: np.ndarray
    dst_start: np.ndarray
    accept: np.ndarray
    regex: Optional[str] = None

    @property
    def n_arcs(self) -> int:
        return int(self.arc_src.shape[0])

    @property
    def accepts_empty(self) -> bool:
        return bool(self.accept[0])

    def step(self, state: int, chan: int) -> int:
        """the state after `chan` from `state`, or -1"""
        return self._delta().get((int(state), int(chan)), -1)

    def accepts(self, chans: Sequence[int]) -> bool:
        q = 0
        for c in chans:
            q = self.step(q, c)
            if q < 0:
                return False
        return bool(self.accept[q])

    def _delta(self) -> Dict[Tuple[int, int], int]:
        d = self.__dict__.get("_delta_cache")
        if d is None:
            d = {(int(s), int(c)): int(t) for s, c, t in zip(self.arc_src, self.arc_chan, self.arc_dst)}
            self.__dict__["_delta_cache"] = d
        return d


def _from_arcs(n_states: int, arcs: Sequence[Tuple[int, int, int]], accept: Sequence[bool], regex: Optional[str]) -> Automaton:
    """(src, chan, dst) triples in any order -> the Automaton, arcs in their stated order"""
    arr = np.asarray(sorted((d, s, c) for s, c, d in arcs), dtype=np.int64).reshape(-1, 3)
    dst = arr[:, 0]
    return Automaton(int(n_states), arr[:, 1].astype(np.int32), arr[:, 2].astype(np.int32), dst.astype(np.int32),
                     np.searchsorted(dst, np.arange(n_states + 1)).astype(np.int32), np.asarray(accept, dtype=np.int32), regex)


# ---------------------------------------------------------------------------------------------------------------- the parser
# AST: ("set", frozenset of labels) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, m, n or None)
class _Parser:
    def __init__(self, regex: str, charset: Sequence[str]):
        self.s, self.i = regex, 0
        self.index = {c: k for k, c in enumerate(charset) if isinstance(c, str) and len(c) == 1}
        self.all = frozenset(self.index.values())
        self._escapes: Dict[str, frozenset] = {}

    def error(self, what: str, pos: Optional[int] = None):
        pos = self.i if pos is None else pos
        return ValueError(f"pattern {self.s!r}: {what} at position {pos}")

    def escape_set(self, e: str) -> frozenset:
        """the charset characters `\\d`, `\\w` or `\\s` holds: exactly those Python's re.fullmatch accepts"""
        if e not in self._escapes:
            rx = _re.compile("\\" + e)
            self._escapes[e] = frozenset(k for c, k in self.index.items() if rx.fullmatch(c))
        return self._escapes[e]

    def literal(self, ch: str, pos: int) -> int:
        if ch not in self.index:
            raise ValueError(f"pattern {self.s!r}: the literal {ch!r} at position {pos} is not a single-character entry of the charset")
        return self.index[ch]

    def parse(self):
        node = self.alt()
        if self.i < len(self.s):
            raise self.error(f"unexpected {self.s[self.i]!r}")
        return node

    def alt(self):
        parts = [self.cat()]
        while self.i < len(self.s) and self.s[self.i] == "|":
            self.i += 1
            parts.append(self.cat())
        return parts[0] if len(parts) == 1 else ("alt", parts)

    def cat(self):
        parts = []
        while self.i < len(self.s) and self.s[self.i] not in "|)":
            parts.append(self.repeat())
        return parts[0] if len(parts) == 1 else ("cat", parts)

    def repeat(self):
        node = self.atom()
        if self.i < len(self.s) and self.s[self.i] in "*+?{":
            c = self.s[self.i]
            if c == "{":
                m = _re.compile(r"\{(\d+)(?:(,)(\d*))?\}").match(self.s, self.i)
                if not m:
                    raise self.error("a malformed repeat")
                lo = int(m.group(1))
                hi = lo if not m.group(2) else (int(m.group(3)) if m.group(3) else None)
                if lo > MAX_REPEAT or (hi is not None and (hi < lo or hi > MAX_REPEAT)):
                    raise self.error(f"a repeat outside 0..{MAX_REPEAT} or with its bounds reversed")
                self.i = m.end()
            else:
                lo, hi = {"*": (0, None), "+": (1, None), "?": (0, 1)}[c]
                self.i += 1
            if self.i < len(self.s) and self.s[self.i] in "*+?{":
                raise self.error("a repeat of a repeat (lazy and possessive repeats are not in the dialect)")
            node = ("rep", node, lo, hi)
        return node

    def atom(self):
        s, i = self.s, self.i
        c = s[i]
        if c == "(":
            self.i += 1
            if s.startswith("?", self.i):
                if not s.startswith("?:", self.i):
                    raise self.error("only (?: ) among the (? ) groups is in the dialect")
                self.i += 2
            node = self.alt()
            if self.i >= len(s) or s[self.i] != ")":
                raise self.error("a group that is not closed", i)
            self.i += 1
            return node
        if c == "[":
            return ("set", self.klass())
        if c == ".":
            self.i += 1
            return ("set", self.all)
        if c == "\\":
            return ("set", self.escaped(False))
        if c in "*+?{":
            raise self.error("nothing to repeat")
        if c in "^$":
            raise self.error("anchors are not in the dialect")
        if c in "]}":
            raise self.error(f"unexpected {c!r}")
        self.i += 1
        return ("set", frozenset((self.literal(c, i),)))

    def escaped(self, in_class: bool) -> frozenset:
        """at a backslash: the set it stands for"""
        i = self.i
        if i + 1 >= len(self.s):
            raise self.error("a backslash at the end")
        e = self.s[i + 1]
        self.i += 2
        if e in "dws":
            return self.escape_set(e)
        if e in _META or not (e.isalnum() or e == "_"):
            return frozenset((self.literal(e, i + 1),))
        raise self.error(f"the escape \\{e} is not in the dialect", i)

    def klass(self) -> frozenset:
        s, start = self.s, self.i
        self.i += 1
        negate = s.startswith("^", self.i)
        self.i += negate
        items, first = set(), True
        while True:
            if self.i >= len(s):
                raise self.error("a class that is not closed", start)
            c = s[self.i]
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            if c == "\\":
                got = self.escaped(True)
                single = len(got) == 1 and s[self.i - 1] not in "dws"
                lo_ch = s[self.i - 1] if single else None
            else:
                lo_ch, self.i = c, self.i + 1
                got = None
            if lo_ch is not None and s.startswith("-", self.i) and self.i + 1 < len(s) and s[self.i + 1] != "]":
                pos = self.i + 1
                hi_ch = s[pos]
                if hi_ch == "\\":
                    if pos + 1 >= len(s) or s[pos + 1] in "dws":
                        raise self.error("a range that ends in a class escape", pos)
                    hi_ch, pos = s[pos + 1], pos + 1
                self.i = pos + 1
                if ord(hi_ch) < ord(lo_ch):
                    raise self.error(f"the range {lo_ch}-{hi_ch} is reversed", pos)
                items |= {k for ch, k in self.index.items() if ord(lo_ch) <= ord(ch) <= ord(hi_ch)}
            elif got is not None:
                items |= got
            else:
                items.add(self.literal(lo_ch, self.i - 1))
        return frozenset(self.all - items) if negate else frozenset(items)


# ------------------------------------------------------------------------------------------------------- Thompson's construction
class _NFA:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.arcs: List[List[Tuple[frozenset, int]]] = []

    def state(self) -> int:
        self.eps.append([])
        self.arcs.append([])
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        """-> (entry, exit) of the fragment"""
        kind = node[0]
        if kind == "set":
            a, b = self.state(), self.state()
            if node[1]:
                self.arcs[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = b = self.state()
            for part in node[1]:
                x, y = self.build(part)
                self.eps[b].append(x)
                b = y
            return a, b
        if kind == "alt":
            a, b = self.state(), self.state()
            for part in node[1]:
                x, y = self.build(part)
                self.eps[a].append(x)
                self.eps[y].append(b)
            return a, b
        _, sub, lo, hi = node
        a = b = self.state()
        for _ in range(lo):                                               # the required copies
            x, y = self.build(sub)
            self.eps[b].append(x)
            b = y
        if hi is None:                                                    # then a star
            x, y = self.build(sub)
            loop, out = self.state(), self.state()
            self.eps[b].append(loop)
            self.eps[loop] += [x, out]
            self.eps[y].append(loop)
            return a, out
        out = self.state()
        for _ in range(hi - lo):                                          # then the optional copies, each of which may leave
            x, y = self.build(sub)
            self.eps[b] += [x, out]
            b = y
        self.eps[b].append(out)
        return a, out

    def closure(self, states) -> frozenset:
        seen, stack = set(states), list(states)
        while stack:
            for t in self.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)


def _determinise(nfa: _NFA, entry: int, exit_: int, regex: str):
    """the subset construction -> (delta: list of {label: state}, accept: list of bool); ValueError past MAX_STATES or MAX_ARCS (both
    are checked here, before the minimisation, so that an expression that blows up is refused while it is still cheap)"""
    start = nfa.closure((entry,))
    index, order, delta = {start: 0}, [start], []
    k = n_arcs = 0
    while k < len(order):
        moves: Dict[int, set] = {}
        for s in order[k]:
            for labels, t in nfa.arcs[s]:
                for lab in labels:
                    moves.setdefault(lab, set()).add(t)
        row, memo = {}, {}
        for lab in sorted(moves):
            key = frozenset(moves[lab])
            nxt = memo.get(key)
            if nxt is None:
                nxt = memo[key] = nfa.closure(key)
            if nxt not in index:
                if len(order) >= MAX_STATES:
                    raise ValueError(f"pattern {regex!r}: more than {MAX_STATES} states")
                index[nxt] = len(order)
                order.append(nxt)
            row[lab] = index[nxt]
        delta.append(row)
        n_arcs += len(row)
        if n_arcs > MAX_ARCS:
            raise ValueError(f"pattern {regex!r}: more than {MAX_ARCS} arcs")
        k += 1
    return delta, [exit_ in s for s in order]


def _trim_and_minimise(delta, accept):
    """dead states (from which no accepting state is reached) dropped, equivalent states merged, states renumbered breadth-first from
    the start over ascending labels -> (delta, accept) again; a language that is empty keeps its start state alone"""
    n = len(delta)
    back: List[List[int]] = [[] for _ in range(n)]
    for s, row in enumerate(delta):
        for t in row.values():
            back[t].append(s)
    live, stack = set(q for q in range(n) if accept[q]), [q for q in range(n) if accept[q]]
    while stack:
        for s in back[stack.pop()]:
            if s not in live:
                live.add(s)
                stack.append(s)
    if 0 not in live:
        return [{}], [False]
    delta = [{lab: t for lab, t in row.items() if t in live} if s in live else {} for s, row in enumerate(delta)]
    block = [1 if accept[q] else 0 for q in range(n)]
    states = sorted(live)
    while True:                                                           # Moore: refine by (block, the blocks the labels lead to)
        sig = {q: (block[q], tuple(sorted((lab, block[t]) for lab, t in delta[q].items()))) for q in states}
        names: Dict = {}
        new = {q: names.setdefault(sig[q], len(names)) for q in states}
        if len(names) == len(set(block[q] for q in states)):
            break
        for q in states:
            block[q] = new[q]
    for q in states:
        block[q] = new[q]
    rep: Dict[int, int] = {}
    for q in states:
        rep.setdefault(block[q], q)
    order, seen = [block[0]], {block[0]: 0}
    k = 0
    while k < len(order):
        for lab, t in sorted(delta[rep[order[k]]].items()):
            if block[t] not in seen:
                seen[block[t]] = len(order)
                order.append(block[t])
        k += 1
    out_delta = [{lab: seen[block[t]] for lab, t in delta[rep[bk]].items()} for bk in order]
    return out_delta, [bool(accept[rep[bk]]) for bk in order]


def compile_pattern(regex: str, charset: Sequence[str]) -> Automaton:
    """The minimal deterministic automaton of `regex` (the dialect of this module's docstring) over the single-character entries of
    `charset` (arc channel = the entry's index + 1).  ValueError for a syntax error (with its position), a literal outside the
    charset (naming it), more than 4096 states or more than 1 << 20 arcs during the subset construction."""
    if not isinstance(regex, str):
        raise ValueError(f"pattern {regex!r}: an expression is a string")
    ast = _Parser(regex, list(charset)).parse()
    nfa = _NFA()
    entry, exit_ = nfa.build(ast)
    delta, accept = _trim_and_minimise(*_determinise(nfa, entry, exit_, regex))
    return _from_arcs(len(delta), [(s, lab + 1, t) for s, row in enumerate(delta) for lab, t in row.items()], accept, regex)


def words_automaton(words: Sequence[Sequence[int]]) -> Automaton:
    """The trie-shaped automaton of a word list: words are sequences of emission channels (label + 1), as the lexicon decoder takes
    them; the states are the distinct prefixes in breadth-first order ((length, channels) ascending), state 0 the empty one.  Not
    minimised: every word ends in a state of its own."""
    words = [tuple(int(c) for c in z) for z in words]
    nodes = sorted({z[:k] for z in words for k in range(1, len(z) + 1)}, key=lambda g: (len(g), g))
    if len(nodes) + 1 > MAX_STATES:
        raise ValueError(f"words_automaton: {len(nodes) + 1} states, the limit is {MAX_STATES}")
    index = {(): 0}
    index.update({g: i + 1 for i, g in enumerate(nodes)})
    ends = set(words)
    return _from_arcs(len(index), [(index[g[:-1]], g[-1], index[g]) for g in nodes], [g in ends for g in [()] + nodes], None)


# ------------------------------------------------------------------------------------------------------------ the host check
def pattern_tables(auto: Automaton, V: int) -> Tuple[int, int]:
    """The host check of an automaton's tables (the kernels only clamp) -> (n_states, n_arcs).  ValueError for the size limits
    (4096 states, 1 << 20 arcs, V above 15360), arcs that are not sorted by (dst, src, chan) or a dst_start that is not their index,
    a state or a channel outside its range (channels: 1..V-1), two arcs with the same (src, chan), a state that the start does not
    reach, or one from which no accepting state is reached."""
    S = int(auto.n_states)
    src, chan, dst, ds, acc = (np.asarray(getattr(auto, k)).astype(np.int64).reshape(-1)
                               for k in ("arc_src", "arc_chan", "arc_dst", "dst_start", "accept"))
    A = int(src.shape[0])
    if not 1 <= S <= MAX_STATES:
        raise ValueError(f"pattern: {S} states, the limits are 1..{MAX_STATES}")
    if A > MAX_ARCS:
        raise ValueError(f"pattern: {A} arcs, the limit is {MAX_ARCS}")
    if not 2 <= int(V) <= MAX_V:
        raise ValueError(f"pattern: V {V} outside 2..{MAX_V}")
    if chan.shape[0] != A or dst.shape[0] != A or ds.shape[0] != S + 1 or acc.shape[0] != S:
        raise ValueError("pattern: the tables must hold one entry per arc, n_states + 1 offsets and one flag per state")
    if A and (int(src.min()) < 0 or int(src.max()) >= S or int(dst.min()) < 0 or int(dst.max()) >= S):
        raise ValueError(f"pattern: an arc with a state outside 0..{S - 1}")
    if A and (int(chan.min()) < 1 or int(chan.max()) > V - 1):
        raise ValueError(f"pattern: a channel outside 1..{V - 1}")
    key = (dst * S + src) * int(V) + chan
    if A > 1 and bool((key[1:] <= key[:-1]).any()):
        raise ValueError("pattern: the arcs are not sorted by (dst, src, chan), or one of them repeats")
    if not np.array_equal(ds, np.searchsorted(dst, np.arange(S + 1))):
        raise ValueError("pattern: dst_start does not hold the first arc into every state (and n_arcs at the end)")
    out = src * int(V) + chan
    if A and np.unique(out).shape[0] != A:
        raise ValueError("pattern: two arcs with the same (src, chan): the automaton is not deterministic")
    fwd = np.zeros(S, dtype=bool)
    fwd[0] = True
    bwd = acc != 0
    for _ in range(S):                                                     # reachability by relaxation: at most S rounds
        f2, b2 = fwd.copy(), bwd.copy()
        f2[dst[fwd[src]]] = True
        b2[src[bwd[dst]]] = True
        if np.array_equal(f2, fwd) and np.array_equal(b2, bwd):
            break
        fwd, bwd = f2, b2
    if not bool(fwd.all()):
        raise ValueError("pattern: a state that the start state does not reach")
    if not bool(bwd.all()):
        raise ValueError("pattern: the accepting set is unreachable from some state (or empty)")
    return S, A


def pattern_upload(auto: Automaton, V: int, device):
    """The automaton checked (pattern_tables) and put on `device`: what pattern_decode and pattern_search take as `tables`.  The
    caller owns the result; nothing is kept here, a changed automaton needs a new upload."""
    S, A = pattern_tables(auto, V)
    tb = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(getattr(auto, k)), dtype=np.int32)).to(device) for k in _PATTERN_FIELDS}
    if A == 0:                                                             # a pointer the library can be handed
        tb["arc_src"] = tb["arc_chan"] = torch.zeros((1,), dtype=torch.int32, device=device)
    tb.update(n_states=S, n_arcs=A, accepts_empty=bool(auto.accepts_empty), V=int(V), device=torch.device(device), regex=auto.regex)
    return tb


def _check(emissions, tables, what: str):
    if not emissions.is_cuda:
        raise RuntimeError(f"dtlr_amd: emissions must live on the GPU (no CPU path; got device {emissions.device})")
    if emissions.dim() != 3:
        raise ValueError(f"{what}: emissions must be [B, T, V]")
    emissions = emissions.float().contiguous()
    V = int(emissions.shape[2])
    if tables["V"] != V or tables["device"] != emissions.device:
        raise ValueError(f"{what}: tables uploaded for V = {tables['V']} on {tables['device']}, emissions have V = {V} on {emissions.device}")
    return emissions


@_lib.op
def pattern_decode(emissions, spans, tables, bonus: float = 0.0):
    """The best string of the automaton's language over every span (dtlr_pattern_decode; semantics: DESIGN.md section 19), exact.
    emissions [B,T,V] fp32 CUDA probabilities (channel 0 = blank); spans: HOST [n,3] integers (line, first frame, one past the last),
    checked here before the upload; tables = pattern_upload(automaton, V, device); bonus: what every character adds to the key that
    candidates are compared by (the returned score is without it).
    -> dict(labels [n,Lcap] int32 channels, left-packed and padded with -1, Lcap = the longest span; length [n] int32, -1 where no
    string of the language fits; score [n] fp64, -inf there; base [n] fp64) on the device.  The spans go out in chunks whose workspace
    stays under PATTERN_WORKSPACE_LIMIT; ValueError, naming the sizes, when a single span cannot fit."""
    emissions = _check(emissions, tables, "pattern_decode")
    bonus = float(bonus)
    if not math.isfinite(bonus):
        raise ValueError(f"pattern_decode: bonus {bonus} is not finite")
    B, T, V = emissions.shape
    S, A, dev = tables["n_states"], tables["n_arcs"], emissions.device
    sp = torch.as_tensor(spans, dtype=torch.int64, device="cpu").reshape(-1, 3)
    n = int(sp.shape[0])
    if n and (int(sp[:, 0].min()) < 0 or int(sp[:, 0].max()) >= B or int(sp[:, 1].min()) < 0 or int(sp[:, 2].max()) > T
              or bool((sp[:, 1] > sp[:, 2]).any())):
        raise ValueError(f"pattern_decode: span table outside emissions [{B}, {T}, {V}]")
    Lcap = int((sp[:, 2] - sp[:, 1]).max()) if n else 0
    out = dict(labels=torch.empty((n, Lcap), dtype=torch.int32, device=dev), length=torch.empty((n,), dtype=torch.int32, device=dev),
               score=torch.empty((n,), dtype=torch.float64, device=dev), base=torch.empty((n,), dtype=torch.float64, device=dev))
    if n == 0:
        return out
    L_ = _lib.lib()
    per_group = _lib.query(L_, "dtlr_pattern_decode_workspace_bytes", 1, S, A, Lcap)
    if per_group > PATTERN_WORKSPACE_LIMIT:
        raise ValueError(f"pattern_decode: one span of {Lcap} frames against {S} states and {A} arcs needs {per_group} bytes of "
                         f"workspace, the limit is {PATTERN_WORKSPACE_LIMIT}")
    chunk = max(int(PATTERN_WORKSPACE_LIMIT // per_group), 1)                # workgroups, hence spans, whose workspace fits the limit
    if chunk >= _GRID:                                                       # the grid never grows past 2048 workgroups: one launch
        chunk = n
    sp_d = sp.to(torch.int32).to(dev)
    for k0 in range(0, n, chunk):
        m = min(chunk, n - k0)
        tmax = int((sp[k0: k0 + m, 2] - sp[k0: k0 + m, 1]).max())
        ws = torch.empty(max(_lib.query(L_, "dtlr_pattern_decode_workspace_bytes", m, S, A, tmax), 16) // 8, dtype=torch.float64, device=dev)
        _lib.launch(L_, "dtlr_pattern_decode", emissions.data_ptr(), B, T, V, sp_d[k0:].data_ptr(), m, tmax, tables["arc_src"].data_ptr(),
                    tables["arc_chan"].data_ptr(), tables["dst_start"].data_ptr(), tables["accept"].data_ptr(), S, A, bonus,
                    out["labels"][k0:].data_ptr(), Lcap, out["length"][k0:].data_ptr(), out["score"][k0:].data_ptr(),
                    out["base"][k0:].data_ptr(), ws.data_ptr())
    return out


@_lib.op
def pattern_search(emissions, tables, min_conf: float = 0.5, H: int = 4, bonus: Optional[float] = None):
    """Every occurrence of the automaton's language in every line, free start and end, best first (dtlr_pattern_search; semantics:
    DESIGN.md section 19), selection included, one launch per chunk of lines.  emissions [B,T,V] fp32 CUDA probabilities; tables =
    pattern_upload(automaton, V, device); a hit needs ratio >= nchar ln(min_conf) (min_conf 0: no bar); H: hits per line, 1..16;
    bonus: what every character adds to the key hits grow and are ranked by; None = -ln(min_conf), 0 when min_conf is 0: a hit then
    grows over a character exactly when that character alone clears the bar.
    -> dict(count [B] int32, start / end / nchar [B,H] int32 padded with -1, ratio [B,H] fp64 padded with 0) on the device.
    ValueError for an automaton that accepts the empty string, min_conf outside 0..1, H outside 1..16."""
    emissions = _check(emissions, tables, "pattern_search")
    if tables["accepts_empty"]:
        raise ValueError(f"pattern_search: the pattern {tables.get('regex')!r} accepts the empty string: it is found everywhere")
    H, min_conf = int(H), float(min_conf)
    if not 1 <= H <= MAX_HITS:
        raise ValueError(f"pattern_search: H {H} outside 1..{MAX_HITS}")
    if not 0.0 <= min_conf <= 1.0:
        raise ValueError(f"pattern_search: min_conf {min_conf} outside 0..1")
    ln = math.log(min_conf) if min_conf > 0 else float("-inf")
    bonus = default_bonus(min_conf) if bonus is None else float(bonus)
    if not math.isfinite(bonus):
        raise ValueError(f"pattern_search: bonus {bonus} is not finite")
    B, T, V = emissions.shape
    S, A, dev = tables["n_states"], tables["n_arcs"], emissions.device
    out = dict(count=torch.empty((B,), dtype=torch.int32, device=dev), start=torch.empty((B, H), dtype=torch.int32, device=dev),
               end=torch.empty((B, H), dtype=torch.int32, device=dev), nchar=torch.empty((B, H), dtype=torch.int32, device=dev),
               ratio=torch.empty((B, H), dtype=torch.float64, device=dev))
    if B == 0:
        return out
    if T == 0:
        raise ValueError("pattern_search: emissions without frames")
    L_ = _lib.lib()
    per_group = _lib.query(L_, "dtlr_pattern_search_workspace_bytes", 1, S, A, T)
    if per_group > PATTERN_WORKSPACE_LIMIT:
        raise ValueError(f"pattern_search: one line of {T} frames against {S} states and {A} arcs needs {per_group} bytes of "
                         f"workspace, the limit is {PATTERN_WORKSPACE_LIMIT}")
    chunk = max(int(PATTERN_WORKSPACE_LIMIT // per_group), 1)
    if chunk >= _GRID:
        chunk = B
    for b0 in range(0, B, chunk):
        m = min(chunk, B - b0)
        ws = torch.empty(max(_lib.query(L_, "dtlr_pattern_search_workspace_bytes", m, S, A, T), 16) // 8, dtype=torch.float64, device=dev)
        _lib.launch(L_, "dtlr_pattern_search", emissions[b0:].data_ptr(), m, T, V, tables["arc_src"].data_ptr(), tables["arc_chan"].data_ptr(),
                    tables["dst_start"].data_ptr(), tables["accept"].data_ptr(), S, A, bonus, ln, H, out["count"][b0:].data_ptr(),
                    out["start"][b0:].data_ptr(), out["end"][b0:].data_ptr(), out["ratio"][b0:].data_ptr(), out["nchar"][b0:].data_ptr(),
                    ws.data_ptr())
    return out


def default_bonus(min_conf: float) -> float:
    """the length bonus that goes with a confidence bar: -ln(min_conf), 0 when min_conf is 0"""
    return -math.log(min_conf) if min_conf > 0 else 0.0
