"""Contextual biasing of the transducer beam search: phrase lists as prefix tries (shallow fusion).

A ``ContextGraph`` holds the phrases a user wants the search to prefer - contact names, commands, a meeting's jargon, in target-speaker
ASR one list per enrolled speaker - as token-id sequences in a trie, with one weight ``w`` > 0: nats added per matched token. Every
hypothesis of the beam search carries a trie state (0, the root, at the start). A non-blank extension by token v moves it:

    step(s, v):  s has a child c on v            -> (c, +w)
                 otherwise d = -pending[s], and
                     the root has a child c on v -> (c, d + w)
                     else                        -> (0, d)

``pending[s] = w * (depth[s] - tdepth[s])`` is the bonus handed out on the way to s that no completed phrase has earned yet (tdepth = depth
of the deepest terminal on the path root..s): it is given back when the match fails, and at the read-out a hypothesis is ranked and
reported with (logp - pending[state]) / len, so a phrase left half-matched earns nothing. A terminal state with children keeps matching
the longer phrase; what it earned so far is committed (its pending is 0). ``pending`` is computed once, here, as a Python float product
and stored as float64: the host loop (decoders.py), the float64 restatement of the tests and the kernel (csrc/search.hip) all read the
array and never recompute it, so their bits agree by construction.

There are NO Aho-Corasick failure links: a failed match restarts at the root with the current token only. With the phrase ``A B A C``
the token sequence ``A B A B A C`` is missed: at the second B the state (after A B A) has no child on B, the match is cancelled, B opens
nothing at the root, and the following ``A C`` is no phrase; failure links would have fallen back to the state after ``A B`` and matched.

The device form is CSR: child_off int32 [S + 1], child_tok int32 [E] ascending within a state, child_to int32 [E] (the graph's own state
ids), pending float64 [S]. ``pack`` concatenates the graphs of a batch and adds base int32 [B] (first row of utterance b's graph, -1: not
biased) and weight float64 [B]. States stay relative to their own graph, in child_to and in the search's per-node array, so repacking for
a new session never invalidates a running one.
"""
import numpy as np


class ContextGraph:
    def __init__(self, phrases, weight):
        """``phrases``: an iterable of non-empty token-id sequences, inserted in the given order, token by token; a new state gets the
        next id when it is created (state 0 is the root); duplicates are ignored. An empty list is allowed: the graph then behaves as no
        graph at all (``empty``). ``weight``: w > 0, nats per matched token."""
        weight = float(weight)
        if not weight > 0 or weight != weight or weight == float("inf"):
            raise ValueError(f"ContextGraph: weight must be a positive finite number, got {weight}")
        self.weight = weight
        children, depth, terminal, tdepth = [{}], [0], [False], [0]
        self.phrases = []
        for phrase in phrases:
            toks = [int(t) for t in phrase]
            if not toks or any(t < 0 for t in toks) or any(int(t) != t for t in phrase):
                raise ValueError(f"ContextGraph: a phrase must be a non-empty sequence of token ids >= 0, got {list(phrase)!r}")
            s = 0
            for t in toks:
                if t not in children[s]:
                    children[s][t] = len(children)
                    children.append({})
                    depth.append(depth[s] + 1)
                    terminal.append(False)
                    tdepth.append(0)
                s = children[s][t]
            if not terminal[s]:
                terminal[s] = True
                self.phrases.append(toks)
        order = sorted(range(len(children)), key=lambda s: depth[s])        # parents before children (ids grow along a path anyway)
        parent = {c: s for s in range(len(children)) for c in children[s].values()}
        for s in order[1:]:
            tdepth[s] = depth[s] if terminal[s] else tdepth[parent[s]]
        self.children, self.depth, self.terminal, self.tdepth = children, depth, terminal, tdepth
        self.pending = np.array([weight * (depth[s] - tdepth[s]) for s in range(len(children))], np.float64)
        off, tok, to = [0], [], []
        for s in range(len(children)):
            for t in sorted(children[s]):
                tok.append(t)
                to.append(children[s][t])
            off.append(len(tok))
        self.child_off, self.child_tok, self.child_to = np.array(off, np.int32), np.array(tok, np.int32), np.array(to, np.int32)

    @property
    def num_states(self):
        return len(self.children)

    @property
    def empty(self):
        return len(self.children) == 1

    def step(self, s, v):
        """(next state, score delta) of state ``s`` on the non-blank token ``v`` (the module docstring's rule; d + w is one float add)."""
        c = self.children[s].get(int(v))
        if c is not None:
            return c, self.weight
        d = -float(self.pending[s])
        c = self.children[0].get(int(v))
        if c is not None:
            return c, d + self.weight
        return 0, d

    def check(self, blank_id, vocab=None):
        """ValueError if a phrase holds the blank or (``vocab`` given) a token outside [0, vocab)."""
        for t in self.child_tok.tolist():
            if t == int(blank_id):
                raise ValueError(f"ContextGraph: a phrase contains the blank id {blank_id}")
            if vocab is not None and not 0 <= t < int(vocab):
                raise ValueError(f"ContextGraph: token {t} outside the vocabulary [0, {vocab})")
        return self

    def arrays(self):
        """(child_off [S + 1], child_tok [E], child_to [E], pending [S]) as numpy arrays (int32, int32, int32, float64)."""
        return self.child_off, self.child_tok, self.child_to, self.pending

    @classmethod
    def from_text(cls, lines, pieces, weight, boundary=None):
        """The graph of a phrase file (train_tsasr.py --bias_file): one phrase per line; a line whose fields are all integers gives token
        ids, any other line is text, encoded with the tokenizer's ``pieces`` (id -> piece) by greedy longest match; a space becomes the
        boundary piece (``boundary``: its text; default: the piece " " if there is one, else the SentencePiece mark). Blank lines are
        skipped; a line that cannot be encoded raises ValueError naming it."""
        pieces = [str(p) for p in pieces]
        if boundary is None:
            boundary = " " if " " in pieces else "▁"
        ids = {p: i for i, p in enumerate(pieces) if p}
        longest = max((len(p) for p in ids), default=0)
        phrases = []
        for n, raw in enumerate(lines, 1):
            line = raw.strip()
            if not line:
                continue
            fields = line.split()
            if all(f.lstrip("+").isdigit() for f in fields):
                phrases.append([int(f) for f in fields])
                continue
            text, toks, i = boundary.join(fields), [], 0
            while i < len(text):
                for k in range(min(longest, len(text) - i), 0, -1):
                    if text[i:i + k] in ids:
                        toks.append(ids[text[i:i + k]])
                        i += k
                        break
                else:
                    raise ValueError(f"bias phrase on line {n} cannot be encoded with the tokenizer's pieces: {line!r} (at {text[i:]!r})")
            phrases.append(toks)
        return cls(phrases, weight)


def as_list(bias, B):
    """``bias`` (None, one ContextGraph, or a list of B entries each a ContextGraph or None) as a list of B graphs or None; an empty
    graph counts as None."""
    if bias is None:
        return [None] * B
    if isinstance(bias, ContextGraph):
        bias = [bias] * B
    bias = list(bias)
    if len(bias) != B or any(g is not None and not isinstance(g, ContextGraph) for g in bias):
        raise ValueError(f"bias must be a ContextGraph or a list of {B} entries, each a ContextGraph or None")
    return [None if g is None or g.empty else g for g in bias]


_PACKS = {}          # (device, ids of the graphs) -> (the graphs, kept alive so that the ids stay theirs; the packed dict)
_PACKS_MAX = 64


def pack(graphs, device):
    """The device form of a batch's graphs: ``graphs`` = list of B entries, each a ContextGraph or None. Returns a dict of tensors on
    ``device``: child_off int32 [rows], child_tok / child_to int32 [edges], pending float64 [rows] - each distinct graph once, S + 1 rows
    (child_off: shifted to absolute edge indices; pending: one unused 0 behind the states) - base int32 [B] (-1: None) and weight
    float64 [B]; plus rows, edges and base_host (a tuple) for the wrappers' checks. A batch without any graph still gives one root row,
    so that no tensor is empty. Cached per device, keyed by the identities of the graphs."""
    import torch
    graphs = [None if g is None or g.empty else g for g in graphs]
    key = (str(device), tuple(id(g) if g is not None else 0 for g in graphs))
    hit = _PACKS.get(key)
    if hit is not None:
        return hit[1]
    off, tok, to, pend, base, weight, first = [], [], [], [], [], [], {}
    rows = edges = 0
    for g in graphs:
        if g is None:
            base.append(-1)
            weight.append(0.0)
            continue
        if id(g) not in first:
            first[id(g)] = rows
            off.append(g.child_off.astype(np.int64) + edges)
            tok.append(g.child_tok)
            to.append(g.child_to)
            pend.append(np.concatenate([g.pending, np.zeros(1)]))
            rows += g.num_states + 1
            edges += int(g.child_tok.shape[0])
        base.append(first[id(g)])
        weight.append(g.weight)
    if rows == 0:
        off, tok, to, pend, rows, edges = [np.zeros(2, np.int64)], [np.full(1, -1, np.int32)], [np.zeros(1, np.int32)], [np.zeros(2)], 2, 1
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate(a).astype(dt))).to(device)  # noqa: E731
    out = dict(child_off=t(off, np.int32), child_tok=t(tok, np.int32), child_to=t(to, np.int32), pending=t(pend, np.float64),
               base=torch.tensor(base, dtype=torch.int32).to(device), weight=torch.tensor(weight, dtype=torch.float64).to(device),
               rows=rows, edges=edges, base_host=tuple(base))
    if len(_PACKS) >= _PACKS_MAX:
        _PACKS.pop(next(iter(_PACKS)))
    _PACKS[key] = (list(graphs), out)
    return out
