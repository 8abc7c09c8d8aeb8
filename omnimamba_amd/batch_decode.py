"""Continuous batching of decode requests of different prompt and answer lengths (MMU questions: 4 + 729 image positions + a question of
any length, answers that end at EOS).

The states live in a pool of ``max_batch`` slots.  A request is admitted FIFO into a free slot: a batch-1 prefill at its exact length
writes the slot (views of the pool: no padding ever reaches a recurrent state), its first id is sampled from the prefill logits, and it
joins the step.  The step runs the live rows in the smallest bucket of {1, 2, 4, ..., max_batch} that holds them; every row carries its
own position and its slot (``InferenceParams.state_indices``), empty rows of the bucket carry slot -1 and leave every state alone.  A row
retires on EOS or at its own ``max_length``; its slot goes to the next request.  Retiring and admitting rewrite the small row buffers
(ids, positions, slots) and never move a state.  With ``cg=True`` one step graph is captured per bucket.

Multi-turn (MMU follow-ups): a request may carry the ``DecodeState`` its previous turn left (``return_states=True``).  Admission copies it
into the free slot and extends the slot by the pending id and the new turn's tokens (Mamba2's extend path: the conversation is never
re-prefilled), then the request decodes like any other.

Ragged prefill (both off by default).  ``prefill_batch`` > 1: the plain requests at the head of the queue that find a free slot at the
same moment are admitted by ONE right-padded prefill (``InferenceParams.seq_lens``: the kernels leave every row's states as after its
own length) into the first rows of a staging cache, which are then copied into their slots.  ``prefill_bucket`` > 0 with ``cg``: a
prompt longer than the exact-length capture limit replays a captured batch-1 prefill of its length rounded up to the bucket.

Ragged extend (off by default).  ``extend_batch`` > 1: the continued requests at the head of the queue that find a free slot at the same
moment are admitted by ONE right-padded extend straight on their pool slots (``InferenceParams.state_indices`` + ``extend_lens``:
every row's states end up as after its own pending id and turn).
"""
from __future__ import annotations

from collections import deque
from dataclasses import dataclass, replace
from typing import List, Tuple

import torch

from . import generation as G
from .generation import InferenceParams, PrefillGraph, MAX_PREFILL_GRAPHS, _prefill_graph_ok, sample
from . import sampling as _sampling
from .sampling import (MAX_EDITS, SamplingParams, TokenLogprobs, apply_logit_edits, apply_token_mask, edit_list, has_count_penalties, has_edits,
                       mask_words, pack_count_penalties, pack_edits, pack_rows, sample_rows)

# A draw with presence / frequency penalties takes the fused path (sampling.penalty_edits + the edit launch) while the rows' user width plus
# the ids their requests have sampled so far fit this many entries; past it the draw edits a copy.  Equal to MAX_EDITS; a name of its own
# so that a test can lower it.
PENALTY_FUSED_MAX = MAX_EDITS


@dataclass
class DecodeState:
    """What a finished request leaves for its next turn: the recurrent state of one sequence after `seqlen` positions.
    layers: per layer (in layer order) the batch-1 (conv_state, ssm_state) copies; pending_id: the last sampled id, which the model
    has not consumed yet (the next turn starts with it, at position seqlen); task and dtype: of the cache it was copied from."""
    layers: List[Tuple[torch.Tensor, torch.Tensor]]
    seqlen: int
    pending_id: int
    task: str
    dtype: torch.dtype


def _buckets(max_batch):
    b, out = 1, []
    while b < max_batch:
        out.append(b)
        b *= 2
    return out + [max_batch]


class _Bucket:
    """Static row buffers of one bucket size and the InferenceParams that point the step at the pool through them; with cg the
    captured step (empty rows only while it is warmed up and captured: no state is touched)."""

    def __init__(self, model, pool, nb, max_seqlen, task, cg, mempool):
        dev = next(iter(model.parameters())).device
        self.nb = nb
        self.input_ids = torch.zeros(nb, 1, dtype=torch.long, device=dev)
        self.position_ids = torch.zeros(nb, 1, dtype=torch.long, device=dev)
        self.slots = torch.full((nb,), -1, dtype=torch.int32, device=dev)
        # seqlen_offset > 0 selects the step branch everywhere; its value is not read by the step itself
        self.ip = InferenceParams(max_seqlen=max_seqlen, max_batch_size=nb, seqlen_offset=1, key_value_memory_dict=pool,
                                  state_indices=self.slots)
        self.task = task
        self.model = model
        self.samp = None        # per-request sampling (decode_ragged(sampling=...)): the rows' setting tensors, made on first use
        self.graph = None
        if cg:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):
                    self._fwd()
                s.synchronize()
            torch.cuda.current_stream().wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            with G.capture(self.graph, pool=mempool):
                self.logits = self._fwd()

    def _fwd(self):
        out = self.model(self.input_ids, None, position_ids=self.position_ids, task=self.task, inference_params=self.ip,
                         num_last_tokens=1)
        return (out.t2i_logits if self.task == "t2i" else out.mmu_logits).squeeze(1)

    def run(self):
        if self.graph is None:
            return self._fwd()
        self.graph.replay()
        return self.logits

    def row_settings(self):
        """Static per-row setting tensors of sample_rows next to `slots`: rewritten when the rows change, steps / history_lens advanced
        on the device in between; `active` is 0 for the padding rows."""
        if self.samp is None:
            dev = self.input_ids.device
            self.samp = pack_rows([SamplingParams()] * self.nb, dev)
            self.samp = {k: v.clone() for k, v in self.samp.items()}      # (pack_rows hands out rows of shared tensors)
            self.samp["active"] = torch.zeros(self.nb, dtype=torch.int32, device=dev)
            self.samp["history_lens"] = torch.zeros(self.nb, dtype=torch.int32, device=dev)
            self.samp["out"] = torch.zeros(self.nb, dtype=torch.long, device=dev)
        return self.samp

    def row_edits(self, width):
        """Static per-row edit tensors (nb, width) of sample_rows next to the row settings: rewritten when the rows (or what is banned in
        them) change; made anew when a call needs another width."""
        st = self.row_settings()
        if "edit_ids" not in st or st["edit_ids"].shape[1] != width:
            st.update(pack_edits([SamplingParams()] * self.nb, self.input_ids.device, width=width))
        return st

    def row_penalties(self, need=None):
        """Static frequency / presence / count_start rows next to the row settings, and (need given) the static merged edit buffers that
        sampling.penalty_edits writes for the edit launch: a power of two wide, at least `need` and at most MAX_EDITS, made anew only when
        the width has to grow."""
        st, dev = self.row_settings(), self.input_ids.device
        if "frequency" not in st:
            st.update({k: v.clone() for k, v in pack_count_penalties([SamplingParams()] * self.nb, dev).items()})
            st["count_start"] = torch.zeros(self.nb, dtype=torch.int32, device=dev)
        if need is not None and ("merged" not in st or st["merged"]["edit_ids"].shape[1] < need):
            w = 1
            while w < need:
                w *= 2
            w = min(w, MAX_EDITS)
            st["merged"] = {"edit_ids": torch.zeros(self.nb, w, dtype=torch.long, device=dev), "edit_vals": torch.zeros(self.nb, w, device=dev),
                            "edit_lens": torch.zeros(self.nb, dtype=torch.int32, device=dev), "edit_mode": torch.zeros(self.nb, dtype=torch.int32, device=dev)}
        return st

    def row_masks(self, words):
        """Static token-mask buffers of guided decoding next to the row settings, made on first use: the device (nb, words) int32 mask the
        masked launch reads, the (nb,) mask_on flags, and ONE pinned host staging buffer the guides' masks are gathered in."""
        st, dev = self.row_settings(), self.input_ids.device
        if "token_mask" not in st or st["token_mask"].shape[1] != words:
            st["token_mask"] = torch.full((self.nb, words), -1, dtype=torch.int32, device=dev)
            st["mask_on"] = torch.zeros(self.nb, dtype=torch.int32, device=dev)
            st["mask_stage"] = torch.full((self.nb, words), -1, dtype=torch.int32, pin_memory=dev.type == "cuda")
        return st


def _guide_mask(g, i, words):
    """What guide `g` of request i allows in its next draw: None, or its int32 (words,) CPU mask -- anything else is a ValueError."""
    m = g.mask()
    if m is None:
        return None
    if not isinstance(m, torch.Tensor) or m.dtype != torch.int32 or m.dim() != 1 or m.shape[0] != words or m.device.type != "cpu":
        what = f"{m.dtype} {tuple(m.shape)} on {m.device}" if isinstance(m, torch.Tensor) else type(m).__name__
        raise ValueError(f"decode_ragged: the guide of request {i} must return None or an int32 CPU tensor of ({words},) (sampling.pack_token_mask), got {what}")
    return m


class _RowSampler:
    """decode_ragged(sampling=...): every draw of the call through ONE row-wise launch (sampling.sample_rows), request i with
    params[i].  The n-th id request i samples is drawn at stream position params[i].step0 + n of its seed, whichever rows share the
    launch.  With a repetition penalty somewhere the pool owns a history buffer (max_batch, cap) int64: a slot's history is its request's
    input_ids followed by its sampled ids.  Its length is ids_len[i] + count[i] on the host; the device copy the kernel reads is the
    bucket's static history_lens, advanced on the device between row changes.  With logit edits somewhere (logit_bias, allowed or banned
    ids, min_new_tokens) every draw carries the rows' edit lists, `width` entries wide: the longest list of the call and one entry for the
    EOS ban of min_new_tokens, which is in a row's list while its request has sampled fewer ids than that.  With a presence or frequency
    penalty somewhere the pool owns the history buffer as well and every draw carries the rows' frequency / presence / count_start, the
    length of a request's input_ids: only the ids it sampled in this call count.  Which path such a draw takes is decided on the host from
    `count` and `width` (_draw): penalty_edits + the edit launch while they fit PENALTY_FUSED_MAX entries, a torch-edited copy past it.
    With a guide somewhere (`guides`: per request None or an object with mask() / advance()) every draw with a guided row carries the rows'
    token masks (sampling.sample_rows(token_mask=, mask_on=)): mask() is called once in front of each draw of a guided request, and the
    caller hands every sampled id back through advance()."""

    def __init__(self, c, params, requests, lens, dev, eos=None, guides=None):
        self.c, self.params, self.dev, self.eos = c, params, dev, eos
        self.guides = guides if guides is not None and any(g is not None for g in guides) else None
        self.prev_on = None                        # the mask_on flags the bucket of the last step holds
        self.edit = any(has_edits(p) or p.min_new_tokens > 0 for p in params)
        self.width = 1 + max(len(edit_list(p)[0]) for p in params) if self.edit else 0
        self.count = [0] * len(params)             # ids sampled so far, per request
        self.ids_len = [r[0].shape[1] for r in requests]
        self.requests = requests
        self.pen = any(p.repetition_penalty != 1.0 for p in params)
        self.cpen = any(has_count_penalties(p) for p in params)
        self.hist_on = self.pen or self.cpen       # the pool owns a history buffer
        self.prev = None                           # (bucket size, requests of the rows) of the last step
        if self.hist_on:
            cap = max(c["max_seqlen"], max(l + m for l, m in zip(self.ids_len, lens)))
            h = c.get("history")
            if h is None or h.shape[1] < cap or h.device != dev:
                c["history"] = torch.zeros(c["max_batch"], cap, dtype=torch.long, device=dev)
            self.hist = c["history"]

    def _settings(self, reqs):
        return pack_rows([replace(self.params[i], step0=self.params[i].step0 + self.count[i]) for i in reqs], self.dev)

    def _rows_history(self, rows, reqs):
        """The histories of the pool slots `rows` (device) in row order, as wide as the longest of the requests `reqs` is now: the
        lengths are known on the host (a request's input_ids + the ids it has sampled), so the gather leaves the unused tail alone."""
        w = max(1, max(self.ids_len[i] + self.count[i] for i in reqs))
        return self.hist[:, :w].index_select(0, rows)

    def _bans(self, reqs):
        """Per request of `reqs`: the ids banned on top of its own settings in its next draw -- EOS until it has sampled min_new_tokens ids."""
        return [[self.eos] if self.count[i] < self.params[i].min_new_tokens else [] for i in reqs]

    def _edits(self, reqs):
        return pack_edits([self.params[i] for i in reqs], self.dev, self._bans(reqs), width=self.width)

    def _draw(self, logits, kw, reqs, merged=None):
        """One row-wise draw with the keyword arguments `kw` of sample_rows for rows that belong to the requests `reqs`.  With presence /
        frequency penalties in the call (kw carries frequency, presence and count_start then) the host picks the path: the fused one while
        the user width plus the most ids a request of `reqs` has sampled fit PENALTY_FUSED_MAX entries -- merged(need) hands out the static
        buffers of the merged lists --, past it the plain launch on a copy edited with torch."""
        if not self.cpen:
            return sample_rows(logits, **kw)
        guide = {k: kw[k] for k in ("token_mask", "mask_on") if k in kw}
        cmax = max(self.count[i] for i in reqs)
        need = self.width + cmax
        if need <= PENALTY_FUSED_MAX:
            return sample_rows(logits, **kw, count_max=cmax, merged=None if merged is None else merged(need))
        plain = {k: kw[k] for k in ("top_k", "top_p", "temperature", "min_p", "seeds", "steps", "active", "out") if k in kw}
        work = apply_logit_edits(logits, kw.get("edit_ids"), kw.get("edit_vals"), kw.get("edit_lens"), kw.get("edit_mode"), penalty=kw.get("penalty"),
                                 history=kw["history"], history_lens=kw["history_lens"], frequency=kw["frequency"], presence=kw["presence"],
                                 count_start=kw["count_start"])
        if guide:
            work = apply_token_mask(work, **guide)
        return sample_rows(work, **plain)

    def admit(self, reqs, slots, logits):
        """The first id of the requests `reqs` (just admitted into `slots`) from their prefill / extend logits (len(reqs), vocab)."""
        gk = self._admit_masks(reqs, logits.shape[1])      # (first: a guide's ValueError comes before anything of the draw is launched)
        pk = self._settings(reqs)
        pk.update(gk)
        if self.edit:
            pk.update(self._edits(reqs))
        if self.hist_on:
            rows = torch.tensor(slots, dtype=torch.long).to(self.dev, non_blocking=True)
            for i, s in zip(reqs, slots):
                self.hist[s, :self.ids_len[i]].copy_(self.requests[i][0][0], non_blocking=True)
            hl = torch.tensor([self.ids_len[i] for i in reqs], dtype=torch.long).to(self.dev, non_blocking=True)
            if self.cpen:
                pk.update(pack_count_penalties([self.params[i] for i in reqs], self.dev), count_start=hl.int())
            toks = self._draw(logits, dict(pk, history=self._rows_history(rows, reqs), history_lens=hl.int()), reqs)
            self.hist.index_put_((rows, hl), toks)
        else:
            pk.pop("penalty")
            toks = sample_rows(logits, **pk)
        for i in reqs:
            self.count[i] += 1
        self.prev = None
        return toks

    def advance(self, i, tok):
        """Request i sampled `tok` (a host int)."""
        if self.guides is not None and self.guides[i] is not None:
            self.guides[i].advance(tok)

    def _admit_masks(self, reqs, vocab):
        """The mask keywords of an admission draw: none when no request of `reqs` is masked in it."""
        if self.guides is None:
            return {}
        w = mask_words(vocab)
        ms = [None if self.guides[i] is None else _guide_mask(self.guides[i], i, w) for i in reqs]
        if all(m is None for m in ms):
            return {}
        tm = torch.stack([torch.full((w,), -1, dtype=torch.int32) if m is None else m for m in ms])
        on = torch.tensor([int(m is not None) for m in ms], dtype=torch.int32)
        return {"token_mask": tm.to(self.dev), "mask_on": on.to(self.dev)}

    def _step_masks(self, bk, live, vocab, rows_changed):
        """The mask keywords of a step of a guided call: the live guided rows' masks go into the bucket's pinned staging rows and ONE
        non-blocking copy moves them to the static device mask; mask_on is rewritten only when the rows changed or a guide switched between
        None and a mask.  Reusing the staging buffer is safe because a call with guides reads the sampled ids on the host after every draw
        (decode_ragged's toks.tolist(), which advance() is fed from): the copy of step n is complete before the host writes step n + 1's
        rows."""
        w, nl = mask_words(vocab), len(live)
        ms = [None if self.guides[i] is None else _guide_mask(self.guides[i], i, w) for i, _, _ in live]
        st = bk.row_masks(w)
        on = tuple(int(m is not None) for m in ms)
        for r, m in enumerate(ms):
            if m is not None:
                st["mask_stage"][r].copy_(m)
        if any(on):
            st["token_mask"][:nl].copy_(st["mask_stage"][:nl], non_blocking=True)
        if rows_changed or (bk.nb, on) != self.prev_on:
            st["mask_on"].copy_(torch.tensor(list(on) + [0] * (bk.nb - nl), dtype=torch.int32), non_blocking=True)
            self.prev_on = (bk.nb, on)
        return {"token_mask": st["token_mask"], "mask_on": st["mask_on"]}

    def step(self, bk, live, rows, logits):
        """One id for every live row of bucket `bk` from the step's logits (bk.nb, vocab); rows: the slots of the bucket's rows (device)."""
        st, nl = bk.row_settings(), len(live)
        key = (bk.nb, tuple(i for i, _, _ in live))
        gk = {} if self.guides is None else self._step_masks(bk, live, logits.shape[1], key[:2] != (self.prev or ())[:2])
        if self.edit:
            st = bk.row_edits(self.width)
            key += (tuple(bool(b) for b in self._bans([i for i, _, _ in live])),)
        if self.cpen:
            st = bk.row_penalties()
        if key != self.prev:
            reqs = [i for i, _, _ in live]
            pk = self._settings(reqs)
            if self.edit:
                pk.update(self._edits(reqs))
            if self.cpen:
                pk.update(pack_count_penalties([self.params[i] for i in reqs], self.dev),
                          count_start=torch.tensor([self.ids_len[i] for i in reqs], dtype=torch.int32).to(self.dev, non_blocking=True))
            for k, v in pk.items():
                st[k][:nl].copy_(v)
            st["active"].copy_(torch.tensor([1] * nl + [0] * (bk.nb - nl), dtype=torch.int32), non_blocking=True)
            if self.hist_on:
                st["history_lens"].copy_(torch.tensor([self.ids_len[i] + self.count[i] for i in reqs] + [0] * (bk.nb - nl), dtype=torch.int32),
                                         non_blocking=True)
            self.prev = key
        kw = {k: st[k] for k in ("top_k", "top_p", "temperature", "min_p", "seeds", "steps", "active", "out")}
        kw.update(gk)
        if self.edit:
            kw.update({k: st[k] for k in ("edit_ids", "edit_vals", "edit_lens", "edit_mode")})
        if self.hist_on:
            reqs = [i for i, _, _ in live]
            if self.cpen:
                kw.update({k: st[k] for k in ("frequency", "presence", "count_start")})
            toks = self._draw(logits, dict(kw, penalty=st["penalty"], history=self._rows_history(rows, reqs), history_lens=st["history_lens"]),
                              reqs, merged=lambda need: bk.row_penalties(need)["merged"])[:nl]
            self.hist.index_put_((rows[:nl], st["history_lens"][:nl].long()), toks)
            st["history_lens"].add_(1)
        else:
            toks = sample_rows(logits, **kw)[:nl]
        st["steps"].add_(1)
        for i, _, _ in live:
            self.count[i] += 1
        return toks.clone()      # (`out` is the bucket's static buffer: the next step overwrites it)


class _LogprobLog:
    """decode_ragged(logprobs=...): every draw of the call is followed by ONE sampling.token_logprobs launch over the logits the draw saw
    and the ids it produced, at the largest N among the requests of its rows that asked for a record (none asked: no launch).  What a
    launch returns stays on the device, one part per draw in the order of `drawn`, and is cut into the requests' records through
    `pieces` at the end, as the ids are: nothing here reads the device."""

    def __init__(self, want, dev):
        self.want, self.dev = want, dev               # per request: None, or its N
        self.nmax = max([w for w in want if w is not None], default=0)
        self.parts = []                               # per draw: (rows, N, TokenLogprobs or None)

    def note(self, logits, ids, reqs, active=None):
        """logits (rows, vocab) and ids (rows,) of one draw whose first len(reqs) rows belong to the requests `reqs`; active: the int32
        flags of the rows when logits and ids are those of a whole bucket (its padding rows are 0)."""
        ns = [self.want[i] for i in reqs if self.want[i] is not None]
        if not ns:
            self.parts.append((len(reqs), 0, None))
            return
        self.parts.append((len(reqs), max(ns), _sampling.token_logprobs(logits, ids, top_n=max(ns), active=active)))

    def records(self, pieces):
        """One TokenLogprobs per request (None where none was asked for), row j of it for the request's j-th sampled id."""
        dev, nmax = self.dev, self.nmax
        lp, rk, ti, tl = [], [], [], []
        for rows, n, r in self.parts:
            if r is None:
                lp.append(torch.zeros(rows, device=dev))
                rk.append(torch.zeros(rows, dtype=torch.int32, device=dev))
            else:
                lp.append(r.logprob[:rows])
                rk.append(r.rank[:rows])
            if nmax:
                a = torch.full((rows, nmax), -1, dtype=torch.long, device=dev) if n < nmax else r.top_ids[:rows]
                b = torch.full((rows, nmax), float("-inf"), device=dev) if n < nmax else r.top_logprobs[:rows]
                if 0 < n < nmax:
                    a[:, :n] = r.top_ids[:rows]
                    b[:, :n] = r.top_logprobs[:rows]
                ti.append(a)
                tl.append(b)
        lp, rk = torch.cat(lp), torch.cat(rk)
        ti = torch.cat(ti) if nmax else torch.zeros(lp.shape[0], 0, dtype=torch.long, device=dev)
        tl = torch.cat(tl) if nmax else torch.zeros(lp.shape[0], 0, device=dev)
        out = []
        for w, pc in zip(self.want, pieces):
            if w is None:
                out.append(None)
                continue
            idx = torch.tensor(pc, dtype=torch.long).to(dev)
            out.append(TokenLogprobs(logprob=lp[idx], rank=rk[idx], top_ids=ti[idx, :w], top_logprobs=tl[idx, :w]))
        return out


def _pool_cache(model, max_batch, max_seqlen, task, cg):
    """The slot pool and the per-bucket steps, kept on the model under the rule of generation.decode's `_decoding_cache`: a new device,
    dtype or task, or a larger max_batch / max_length, drops them."""
    p0 = next(iter(model.parameters()))
    c = getattr(model, "_ragged_cache", None)
    if (c is None or (c["device"], c["dtype"], c["task"], c["cg"]) != (p0.device, p0.dtype, task, cg)
            or max_batch > c["max_batch"] or max_seqlen > c["max_seqlen"]):
        c = {"device": p0.device, "dtype": p0.dtype, "task": task, "cg": cg, "max_batch": max_batch, "max_seqlen": max_seqlen,
             "pool": model.allocate_inference_cache(max_batch, max_seqlen, p0.dtype), "buckets": {}, "prefill": {}, "staging": {},
             "mempool": torch.cuda.graphs.graph_pool_handle() if cg else None}
        model._ragged_cache = None       # (the old pool and graphs go before the new ones are captured)
        model._ragged_cache = c
    return c


def _bucket_len(seqlen, bucket, n_pos):
    """Length of the captured bucket a prompt of `seqlen` positions replays, 0 = none (run it eager).  The stack adds the position
    table to the whole padded buffer, so a bucket never reaches past the table's rows: it is clamped to them, and a prompt that does
    not fit the clamped bucket runs eager (and raises there what it raises today)."""
    if bucket <= 0 or seqlen <= G.PREFILL_GRAPH_MAX_LEN or not G._prefill_graphs_enabled():
        return 0
    blen = -(-seqlen // bucket) * bucket
    if n_pos is not None:
        blen = min(blen, n_pos)
    return blen if blen >= seqlen else 0


def _prefill(model, c, slot, emb, task, cg, bucket=0, n_pos=None):
    """Batch-1 prefill of one prompt into pool slot `slot` -> logits (1, vocab).  Eager: straight into views of the slot.  Captured
    (prompts of <= 512 positions, as generation.decode): a PrefillGraph per prompt length on a batch-1 cache of its own, whose states
    are then copied into the slot.  bucket > 0: longer prompts take a captured graph per length bucket (_bucket_len), their true
    length in its static seq_lens buffer; same LRU, same MAX_PREFILL_GRAPHS."""
    seqlen = emb.shape[1]
    blen = _bucket_len(seqlen, bucket, n_pos) if cg else 0
    if cg and (blen or _prefill_graph_ok(seqlen)):
        key = (blen, emb.dtype, "bucket") if blen else (seqlen, emb.dtype)
        pg = c["prefill"].get(key)
        if pg is None:
            if len(c["prefill"]) >= MAX_PREFILL_GRAPHS:
                del c["prefill"][next(iter(c["prefill"]))]
            ip = InferenceParams(max_seqlen=c["max_seqlen"], max_batch_size=1,
                                 key_value_memory_dict=model.allocate_inference_cache(1, c["max_seqlen"], c["dtype"]))
            pg = PrefillGraph(model, ip, 1, blen or seqlen, emb.shape[-1], task, emb.dtype, mempool=c["mempool"], ragged=bool(blen))
        c["prefill"][key] = c["prefill"].pop(key, pg)          # most recently used last
        lg = pg.run(emb)
        src = [t for k in sorted(pg.ip.key_value_memory_dict) for t in pg.ip.key_value_memory_dict[k]]
        dst = [t[slot:slot + 1] for k in sorted(c["pool"]) for t in c["pool"][k]]
        torch._foreach_copy_(dst, src)
        return lg
    ip = InferenceParams(max_seqlen=c["max_seqlen"], max_batch_size=1,
                         key_value_memory_dict={k: tuple(t[slot:slot + 1] for t in v) for k, v in c["pool"].items()})
    out = model(None, emb, position_ids=None, task=task, inference_params=ip, num_last_tokens=1)
    return (out.t2i_logits if task == "t2i" else out.mmu_logits).squeeze(1)


def _prefill_group(model, c, slots, embs, task):
    """ONE right-padded prefill of several prompts -> logits (len(embs), vocab), row j read at the last position of prompt j.  The rows
    run on the first rows of ONE staging cache (the states are batch-leading; it grows to the largest group seen);
    InferenceParams.seq_lens makes every row's states those after its own length, and they are then copied into the pool rows `slots`.  Pad positions of the embedding buffer are zeros."""
    g, dev = len(embs), embs[0].device
    lens_h = [e.shape[1] for e in embs]
    buf = torch.zeros(g, max(lens_h), embs[0].shape[-1], dtype=embs[0].dtype, device=dev)
    for j, e in enumerate(embs):
        buf[j, :lens_h[j]].copy_(e[0])
    if c["staging"].get("rows", 0) < g:
        c["staging"] = {"rows": g, "cache": model.allocate_inference_cache(g, c["max_seqlen"], c["dtype"])}
    st = {k: tuple(t[:g] for t in v) for k, v in c["staging"]["cache"].items()}
    ip = InferenceParams(max_seqlen=c["max_seqlen"], max_batch_size=g, key_value_memory_dict=st,
                         seq_lens=torch.tensor(lens_h, dtype=torch.int32).to(dev, non_blocking=True))
    out = model(None, buf, position_ids=None, task=task, inference_params=ip, num_last_tokens=1)
    rows = torch.tensor(slots, dtype=torch.long).to(dev, non_blocking=True)
    for k in sorted(c["pool"]):
        for dst, src in zip(c["pool"][k], st[k]):
            dst.index_copy_(0, rows, src)
    return (out.t2i_logits if task == "t2i" else out.mmu_logits).squeeze(1)


def _extend(model, c, slot, state, emb, task):
    """Continue a conversation in pool slot `slot`: copy `state` in, then extend the slot by [state.pending_id] + the turn's embeddings
    `emb` (1, P, d) at positions state.seqlen ... (eager, straight into views of the slot) -> logits (1, vocab) of the last position."""
    if state.task != task or state.dtype != c["dtype"]:
        raise ValueError(f"decode_ragged: a {state.task} / {state.dtype} state cannot continue in a {task} / {c['dtype']} cache")
    dst = [t[slot:slot + 1] for k in sorted(c["pool"]) for t in c["pool"][k]]
    torch._foreach_copy_(dst, [t for pair in state.layers for t in pair])
    dev = emb.device
    pend = model.get_input_embeddings()(torch.tensor([[state.pending_id]], dtype=torch.long, device=dev))
    h = torch.cat([pend.to(emb.dtype), emb], dim=1)
    pos = torch.arange(state.seqlen, state.seqlen + h.shape[1], dtype=torch.long, device=dev)[None]
    # the stack adds no position rows to embeddings it is handed with position_ids: they are added here, at the conversation's positions
    h = h + model.backbone.mmu_pos_embed[:, state.seqlen: state.seqlen + h.shape[1]].to(h.dtype)
    ip = InferenceParams(max_seqlen=c["max_seqlen"], max_batch_size=1, seqlen_offset=state.seqlen,
                         key_value_memory_dict={k: tuple(t[slot:slot + 1] for t in v) for k, v in c["pool"].items()})
    out = model(None, h, position_ids=pos, task=task, inference_params=ip, num_last_tokens=1)
    return out.mmu_logits.squeeze(1)


def _extend_group(model, c, slots, states, embs, task):
    """ONE right-padded extend of several conversations -> logits (len(embs), vocab), row j read at the last position of turn j.  The
    states are copied into the pool rows `slots`, which the pass then extends in place through InferenceParams.state_indices; row j is
    [states[j].pending_id] + embs[j] with the position rows from states[j].seqlen on added here (as _extend), zeros behind it, and
    InferenceParams.extend_lens makes every row's states those after its own length."""
    for st in states:
        if st.task != task or st.dtype != c["dtype"]:
            raise ValueError(f"decode_ragged: a {st.task} / {st.dtype} state cannot continue in a {task} / {c['dtype']} cache")
    g, dev = len(embs), embs[0].device
    dst = [t[s:s + 1] for s in slots for k in sorted(c["pool"]) for t in c["pool"][k]]
    torch._foreach_copy_(dst, [t for st in states for pair in st.layers for t in pair])
    lens_h = [1 + e.shape[1] for e in embs]
    pend = model.get_input_embeddings()(torch.tensor([[st.pending_id] for st in states], dtype=torch.long, device=dev))   # (g, 1, d)
    buf = torch.zeros(g, max(lens_h), embs[0].shape[-1], dtype=embs[0].dtype, device=dev)
    pos = torch.zeros(g, max(lens_h), dtype=torch.long)
    for j, (st, e) in enumerate(zip(states, embs)):
        h = torch.cat([pend[j:j + 1].to(e.dtype), e], dim=1)
        buf[j, :lens_h[j]].copy_((h + model.backbone.mmu_pos_embed[:, st.seqlen: st.seqlen + lens_h[j]].to(h.dtype))[0])
        pos[j, :lens_h[j]] = torch.arange(st.seqlen, st.seqlen + lens_h[j])
    # seqlen_offset > 0 selects the extend branch; its value is not read.  position_ids tells the stack that the position rows are in
    ip = InferenceParams(max_seqlen=c["max_seqlen"], max_batch_size=g, seqlen_offset=1, key_value_memory_dict=c["pool"],
                         state_indices=torch.tensor(slots, dtype=torch.int32).to(dev, non_blocking=True),
                         extend_lens=torch.tensor(lens_h, dtype=torch.int32).to(dev, non_blocking=True))
    out = model(None, buf, position_ids=pos.to(dev, non_blocking=True), task=task, inference_params=ip, num_last_tokens=1)
    return out.mmu_logits.squeeze(1)


def _save(c, slot, seqlen, pending_id, task):
    return DecodeState(layers=[tuple(t[slot:slot + 1].clone() for t in c["pool"][k]) for k in sorted(c["pool"])], seqlen=seqlen,
                       pending_id=pending_id, task=task, dtype=c["dtype"])


@torch.inference_mode()
def decode_ragged(requests, model, max_length, *, max_batch=8, task="mmu", eos_token_id=None, top_k=1, top_p=0.0, temperature=1.0,
                  min_p=0.0, cg=True, return_states=False, prefill_batch=1, prefill_bucket=0, extend_batch=1, sampling=None, logprobs=None,
                  guides=None):
    """requests: list of (input_ids (1, Li), input_embeddings (1, Pi, d)); max_length: an int or one per request, with
    generation.decode's meaning.  Returns one LongTensor (1, Li + n_i) per request: what ``decode(input_ids_i, input_embeddings_i,
    model, max_length_i, ...)`` returns for that request alone -- prompt ids, sampled ids, EOS included, and the IndexError of a step
    past the position table (raised before that step is launched).

    A request may also be (input_ids (1, Li), input_embeddings (1, Pi, d), state): the next turn of a conversation whose previous turn
    left `state` (a DecodeState; 'mmu' only).  Its embeddings are the new turn's only; the slot continues from the state at position
    state.seqlen with [state.pending_id] + the new turn, and max_length counts the whole conversation's positions.  Its ids are
    input_ids followed by the sampled ids.  return_states=True: returns (ids_list, states_list), states_list[i] the DecodeState of
    request i when it finished.

    prefill_batch > 1: up to that many plain requests (not continued ones) that are queued while as many slots are free are admitted
    by one right-padded prefill (_prefill_group); admission stays FIFO, a continued request ends the group before it, and nothing
    waits for a larger group.  prefill_bucket > 0 (with cg): prompts longer than generation.PREFILL_GRAPH_MAX_LEN replay a captured
    prefill of their length rounded up to a multiple of it (_prefill).  With both at their defaults nothing changes.

    extend_batch > 1: up to that many continued requests at the head of the queue that find a free slot at the same moment are admitted
    by one right-padded extend on their slots (_extend_group); admission stays FIFO, a plain request ends the group before it, nothing
    waits for a larger group, and the position-table IndexError of every request of the group is raised before anything is launched.  A
    group of one, or one whose turns are all empty (padded length 1: a decode step), is admitted request by request.  1: off.

    sampling: None -- top_k / top_p / min_p / temperature hold for the whole call and the draws go through generation.sample, as ever.  One
    sampling.SamplingParams for all requests, or a list with one per request: request i is sampled with its own settings (a repetition
    penalty over its input_ids and sampled ids among them) and its own random stream -- its n-th sampled id of this call is drawn at
    position step0 + n of its seed, so its ids do not depend on which requests share its steps, on max_batch or on the admission
    order.  Every draw (prefill, extend, grouped or not, and the step) is one row-wise launch (sampling.sample_rows); top_k, top_p,
    min_p and temperature are not read.  A follow-up turn continues its stream when it is given step0 = the ids drawn so far.
    Constraints (SamplingParams.logit_bias, allowed_token_ids, banned_token_ids, min_new_tokens): when a request of the call has any, every
    draw of the call carries the rows' edit lists and the row-wise launch applies them behind the repetition penalty (sampling.sample_rows,
    omk_sample_rows ABI 16); the lists live in static per-bucket tensors that are rewritten only when the rows change.  min_new_tokens bans
    eos_token_id (required then) until the request has sampled that many ids in this call; the rows are repacked on the step where the ban
    ends.  The requests without constraints draw the ids they draw without constrained neighbours; logprobs stay those of the raw logits.
    Presence and frequency penalties (SamplingParams.presence_penalty, frequency_penalty): over the ids the request has sampled IN THIS CALL
    (its input_ids do not count; a follow-up turn starts at zero).  When a request of the call has one, every draw carries the rows'
    penalties: sampling.penalty_edits builds the rows' lists on the device (merged with their own edits, static per-bucket buffers) and the
    edit launch draws -- two launches, no host read -- while the user width plus the ids sampled so far fit PENALTY_FUSED_MAX entries; past
    that the draw edits a copy with sampling.apply_logit_edits.  The ids are the same on both paths.

    logprobs: None -- off.  An int N in [0, 64] for every request, or a list with one entry per request (an int, or None for a request
    that wants no record): the call returns ONE MORE element behind what it returns otherwise (ids_list, logprobs_list) or (ids_list,
    states_list, logprobs_list) -- per request a sampling.TokenLogprobs (None where none was asked for) whose rows are aligned with the
    request's n_i sampled ids, EOS included: logprob (n_i,) and rank (n_i,) of the sampled id, top_ids and top_logprobs (n_i, N_i), the N_i
    most likely tokens (N = 0: shape (n_i, 0)).  All of the RAW logits the draw saw: no temperature, filter or repetition penalty (a greedy
    request has rank 1 everywhere).  Every draw is followed by one sampling.token_logprobs launch at the largest N among its rows; the
    results stay on the device (the model's) until the call returns, no host synchronisation is added, and with cg the launch reads the
    bucket's static logits before the next replay.  The sampled ids and the states are those of the call without logprobs.

    guides: None -- off.  A list with one entry per request: None, or a GUIDE -- any object with mask() -> None or an int32 (ceil(vocab /
    32),) CPU tensor (bit (i & 31) of word (i >> 5) set = token i may be drawn; None = unconstrained for this draw), called once in front of
    every draw of its request, and advance(token_id), called with every id the request samples, in order, EOS included
    (sampling.ChoiceGuide is one; a grammar engine's matcher is another).  Needs `sampling` (the row-wise path).  Every draw of a guided
    request -- prefill, extend, grouped or not, and the step -- carries its mask into the row-wise launch (omk_sample_rows_masked: the mask
    is applied last, behind the penalties and the edits); per bucket a static device mask, the mask_on flags and one pinned staging
    buffer are made on first use.  The call reads the sampled ids on the host after every draw (as with an eos_token_id).  A mask of the
    wrong dtype, shape or device raises ValueError before anything of that draw is launched.  Requests without a guide draw the ids they
    draw without guided neighbours (mask_on 0); logprobs stay those of the raw logits.  A call in which no request has a guide launches
    what the call without `guides` launches."""
    n = len(requests)
    if logprobs is not None:
        want = [logprobs] * n if isinstance(logprobs, int) else list(logprobs)
        if len(want) != n:
            raise ValueError(f"decode_ragged: logprobs is None, an int or a list of {n}, one entry per request")
        for w in want:
            if w is not None and not (isinstance(w, int) and 0 <= w <= _sampling.MAX_TOP_N):
                raise ValueError(f"decode_ragged: a logprobs entry is None or an int in [0, {_sampling.MAX_TOP_N}], got {w!r}")
    if n == 0:
        empty = ([], []) if return_states else []
        return empty if logprobs is None else ((*empty, []) if return_states else ([], []))
    lens = [int(max_length)] * n if isinstance(max_length, int) else [int(m) for m in max_length]
    if len(lens) != n:
        raise ValueError(f"decode_ragged: {len(lens)} max_length values for {n} requests")
    if max_batch < 1:
        raise ValueError("decode_ragged: max_batch must be >= 1")
    if prefill_batch < 1 or prefill_bucket < 0:
        raise ValueError("decode_ragged: prefill_batch must be >= 1 and prefill_bucket >= 0")
    if extend_batch < 1:
        raise ValueError("decode_ragged: extend_batch must be >= 1")
    for r in requests:
        if len(r) not in (2, 3):
            raise ValueError("decode_ragged: every request is (input_ids, input_embeddings) or (input_ids, input_embeddings, state)")
        ids, emb = r[0], r[1]
        if ids.dim() != 2 or ids.shape[0] != 1 or emb.dim() != 3 or emb.shape[0] != 1:
            raise ValueError("decode_ragged: every request is (input_ids (1, L), input_embeddings (1, P, d))")
        if len(r) == 3 and (task != "mmu" or not isinstance(r[2], DecodeState)):
            raise ValueError("decode_ragged: a continued request carries a DecodeState and is an mmu request")
    if sampling is not None:
        sampling = [sampling] * n if isinstance(sampling, SamplingParams) else list(sampling)
        if len(sampling) != n or not all(isinstance(p, SamplingParams) for p in sampling):
            raise ValueError(f"decode_ragged: sampling is one SamplingParams or a list of {n}, one per request")
        if eos_token_id is None and any(p.min_new_tokens > 0 for p in sampling):
            raise ValueError("decode_ragged: min_new_tokens > 0 needs an eos_token_id to keep out of the first ids")
    if guides is not None:
        if sampling is None:
            raise ValueError("decode_ragged: guides need sampling (one SamplingParams or a list): the masks are applied by the row-wise sampler launch")
        guides = list(guides)
        if len(guides) != n:
            raise ValueError(f"decode_ragged: guides is None or a list of {n}, one entry (a guide or None) per request")
        for g in guides:
            if g is not None and not (callable(getattr(g, "mask", None)) and callable(getattr(g, "advance", None))):
                raise ValueError("decode_ragged: a guide is None or an object with mask() and advance(token_id)")
    dev = requests[0][1].device
    if hasattr(model, "prepare_decode"):
        model.prepare_decode(task)
    cfg_ = getattr(model, "cfg", None)
    n_pos = None if cfg_ is None else getattr(cfg_, "t2i_positions" if task == "t2i" else "mmu_positions", None)
    c = _pool_cache(model, max_batch, max(lens), task, cg)
    buckets = _buckets(max_batch)

    def bucket(nb):
        if nb not in c["buckets"]:
            c["buckets"][nb] = _Bucket(model, c["pool"], nb, c["max_seqlen"], task, cg, c["mempool"])
        return c["buckets"][nb]

    rs = None if sampling is None else _RowSampler(c, sampling, requests, lens, dev, eos_token_id, guides)
    # the first id(s) of the requests `reqs` admitted into `slots`, from their prefill / extend logits
    draw = lambda lg, reqs, slots: (sample(lg, top_k=top_k, top_p=top_p, min_p=min_p, temperature=temperature) if rs is None
                                    else rs.admit(reqs, slots, lg))
    lp = None if logprobs is None else _LogprobLog(want, dev)
    if lp is not None:
        draw_ids = draw

        def draw(lg, reqs, slots):
            toks = draw_ids(lg, reqs, slots)
            lp.note(lg, toks, reqs)
            return toks
    last = torch.zeros(c["max_batch"], dtype=torch.long, device=dev)   # last sampled id of every slot: the next step's input
    drawn, n_drawn = [], 0               # every sampled id tensor in order, and how many ids they hold
    pieces = [[] for _ in range(n)]      # per request: the positions of its ids in cat(drawn), in sampling order
    queue, free = deque(range(n)), list(range(max_batch))
    live = []                            # rows of the step: [request, slot, offset]
    guided = rs is not None and rs.guides is not None
    check_eos = eos_token_id is not None or return_states or guided     # (guides are fed the sampled ids: the host reads them every draw)
    states = [None] * n

    def retire(i, s, off, tok):
        free.append(s)
        if return_states:
            states[i] = _save(c, s, off, tok, task)

    def finished(i, tok, off):
        return (eos_token_id is not None and tok == eos_token_id) or off >= lens[i] - 1

    while queue or live:
        while queue and free:                                  # admit FIFO into free slots
            grp = []                                           # the plain requests at the head of the queue that find a slot now
            while prefill_batch > 1 and len(grp) < min(prefill_batch, len(free), len(queue)) and len(requests[queue[len(grp)]]) == 2:
                grp.append(queue[len(grp)])
            xgrp = []                                          # ... and the continued ones (a request is one or the other)
            while (extend_batch > 1 and len(xgrp) < min(extend_batch, len(free), len(queue))
                   and len(requests[queue[len(xgrp)]]) == 3):
                xgrp.append(queue[len(xgrp)])
            if len(grp) > 1:
                for _ in grp:
                    queue.popleft()
                slots = [free.pop(0) for _ in grp]
                toks = draw(_prefill_group(model, c, slots, [requests[i][1] for i in grp], task), grp, slots)   # (len(grp),)
                toks_h = toks.tolist() if check_eos else [None] * len(grp)
                admitted = [(i, s, requests[i][1].shape[1], toks[j:j + 1], toks_h[j]) for j, (i, s) in enumerate(zip(grp, slots))]
            elif len(xgrp) > 1 and any(requests[i][1].shape[1] > 0 for i in xgrp):   # (all turns empty: a decode step, not an extend)
                offs = [requests[i][2].seqlen + 1 + requests[i][1].shape[1] for i in xgrp]
                for i, off in zip(xgrp, offs):
                    if n_pos is not None and off > n_pos:
                        raise IndexError(f"decode_ragged: request {i} continues to position {off - 1}, outside the {task} position table of "
                                         f"{n_pos} rows (StackConfig.{{t2i,mmu}}_positions)")
                for _ in xgrp:
                    queue.popleft()
                slots = [free.pop(0) for _ in xgrp]
                toks = draw(_extend_group(model, c, slots, [requests[i][2] for i in xgrp], [requests[i][1] for i in xgrp], task), xgrp, slots)
                toks_h = toks.tolist() if check_eos else [None] * len(xgrp)
                admitted = [(i, s, off, toks[j:j + 1], toks_h[j]) for j, (i, s, off) in enumerate(zip(xgrp, slots, offs))]
            else:
                i = queue.popleft()
                s = free.pop(0)
                ids, emb = requests[i][:2]
                if len(requests[i]) == 3:
                    st = requests[i][2]
                    off = st.seqlen + 1 + emb.shape[1]
                    if n_pos is not None and off > n_pos:
                        raise IndexError(f"decode_ragged: request {i} continues to position {off - 1}, outside the {task} position table of "
                                         f"{n_pos} rows (StackConfig.{{t2i,mmu}}_positions)")
                    tok = draw(_extend(model, c, s, st, emb, task), [i], [s])
                else:
                    tok = draw(_prefill(model, c, s, emb, task, cg, prefill_bucket, n_pos), [i], [s])   # (1,)
                    off = emb.shape[1]
                admitted = [(i, s, off, tok, int(tok[0]) if check_eos else None)]
            for i, s, off, tok, tok_h in admitted:
                if guided:
                    rs.advance(i, tok_h)
                last[s:s + 1].copy_(tok)
                drawn.append(tok)
                pieces[i].append(n_drawn)
                n_drawn += 1
                if finished(i, tok_h, off):
                    retire(i, s, off, tok_h)
                else:
                    live.append([i, s, off])
        if not live:
            continue
        if n_pos is not None:
            for i, _, off in live:
                if off >= n_pos:
                    raise IndexError(f"decode_ragged: position {off} of request {i} is outside the {task} position table of "
                                     f"{n_pos} rows (StackConfig.{{t2i,mmu}}_positions)")
        nb = next(b for b in buckets if b >= len(live))
        bk = bucket(nb)
        pad = nb - len(live)
        slots_h = [s for _, s, _ in live]
        rows = torch.tensor(slots_h + [0] * pad, dtype=torch.long).to(dev, non_blocking=True)
        bk.input_ids[:, 0] = last.index_select(0, rows)
        bk.position_ids.copy_(torch.tensor([[off] for _, _, off in live] + [[0]] * pad, dtype=torch.long), non_blocking=True)
        bk.slots.copy_(torch.tensor(slots_h + [-1] * pad, dtype=torch.int32), non_blocking=True)
        if rs is None:
            lg = bk.run()[: len(live)]
            toks = sample(lg, top_k=top_k, top_p=top_p, min_p=min_p, temperature=temperature)
            if lp is not None:
                lp.note(lg, toks, [i for i, _, _ in live])
        else:
            lg = bk.run()
            toks = rs.step(bk, live, rows, lg)
            if lp is not None:     # (the bucket's rows: the ids are still in the sampler's static buffer, the padding rows are inactive)
                lp.note(lg, bk.samp["out"], [i for i, _, _ in live], active=bk.samp["active"])
        last.index_copy_(0, rows[: len(live)], toks)
        toks_h = toks.tolist() if check_eos else None
        still = []
        for r, row in enumerate(live):
            i, s, off = row
            row[2] = off = off + 1
            pieces[i].append(n_drawn + r)
            if guided:
                rs.advance(i, toks_h[r])
            if finished(i, toks_h[r] if check_eos else None, off):
                retire(i, s, off, toks_h[r] if check_eos else None)
            else:
                still.append(row)
        drawn.append(toks)
        n_drawn += len(live)
        live = still
    flat = torch.cat(drawn)
    out = [torch.cat([r[0], flat[torch.tensor(pieces[i], device=dev)].view(1, -1).to(r[0].device)], dim=1)
           for i, r in enumerate(requests)]
    res = (out, states) if return_states else out
    if lp is None:
        return res
    recs = lp.records(pieces)
    return (out, states, recs) if return_states else (out, recs)
