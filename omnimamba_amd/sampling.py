"""On-device token sampling: omk_sample behind the reference's `sample` signature
(/root/reference/models/stage2/generation.py:87-121).  One launch, no host scalar after it: usable inside a captured decode step."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Mapping, Optional, Sequence, Tuple, Union

import torch

from . import _capi as K
from ._lib import get_lib

MAX_TOP_K = 64
MAX_EDITS = 512      # entries of one row's edit list the fused launch holds (SAMPLE_EDIT_MAX of sample.hip); longer lists edit a copy


def applies(logits: torch.Tensor, top_k: int, min_p: float = 0.0, top_p: float = 0.0) -> bool:
    """The HIP sampler covers the reference's top_k == 1 short cut, its top_k > 0 branch up to 64 candidates, and its whole-vocabulary
    branch (top_k == 0): the plain multinomial (t2i_generate's default arguments), the top-p cut over all tokens and the min_p filter."""
    try:
        lib = get_lib()
    except RuntimeError:
        return False
    on_lib_device = logits.is_cuda != bool(lib.omk_is_emulated())
    full = top_k == 0 and 0.0 <= min_p < 1.0 and top_p <= 1.0
    return on_lib_device and (1 <= top_k <= MAX_TOP_K or full) and logits.dim() == 2 and logits.stride(1) == 1 and logits.dtype in (torch.float32, torch.bfloat16, torch.float16)


def sample_device(logits: torch.Tensor, top_k: int = 1, top_p: float = 0.0, temperature: float = 1.0, seed: int = 0,
                  step_counter: Optional[torch.Tensor] = None, offset: int = 0, out: Optional[torch.Tensor] = None, min_p: float = 0.0) -> torch.Tensor:
    """(batch, vocab) -> (batch,) int64 ids.  seed / step_counter / offset select the Philox stream: the same triple gives the same
    ids (row b uses its own stream); step_counter is a device int64 scalar tensor read by the kernel (advance it yourself)."""
    lib = get_lib()
    if out is None:
        out = torch.empty(logits.shape[0], dtype=torch.int64, device=logits.device)
    if step_counter is not None:
        assert step_counter.dtype == torch.int64 and step_counter.device == logits.device
    p = K.Sample(logits=K.T(logits), top_k=int(top_k), top_p=float(top_p), temperature=float(temperature), min_p=float(min_p) if top_k == 0 else 0.0, seed=int(seed) & (2 ** 64 - 1),
                 offset=int(offset), step_counter=None if step_counter is None else step_counter.data_ptr())
    p.out_ids.data = out.data_ptr()
    p.out_ids.ndim = 1
    p.out_ids.shape[0] = out.shape[0]
    p.out_ids.stride[0] = out.stride(0)
    K.run(lib, "omk_sample", p, logits)
    return out


# ---- per-request sampling: one set of settings per row of a batch (omk_sample_rows, ABI 14) --------------------------------------------

@dataclass(frozen=True)
class SamplingParams:
    """How ONE request is sampled.  seed and step0 name its random stream: the n-th id the request samples is drawn at stream position
    step0 + n of seed, whatever batch it shares a step with (a follow-up turn continues its stream by passing the number of ids drawn so
    far as step0).  The rules are omk_sample's own; repetition_penalty 1.0 means off.

    Constraints on what the request may emit (off by default; the rule is omk_sample_rows', ABI 16, applied behind the repetition penalty):
    logit_bias -- a mapping or pairs id -> float added to the token's logit (finite, or -inf: a ban); allowed_token_ids -- only these ids
    may be drawn; banned_token_ids -- never drawn; min_new_tokens -- the call's eos_token_id is banned until the request has sampled that
    many ids in the call.  logit_bias is kept as a tuple of (id, value) pairs, the id sets as tuples.

    presence_penalty / frequency_penalty (0.0 = off, both finite): the OpenAI-style penalties over the ids the request has SAMPLED in the call
    (not its prompt) -- a token sampled c > 0 times gets -((frequency_penalty * c) + presence_penalty) added to its logit, behind the
    repetition penalty and together with the request's own edits (omk_penalty_edits, ABI 17)."""
    top_k: int = 1
    top_p: float = 0.0
    min_p: float = 0.0
    temperature: float = 1.0
    repetition_penalty: float = 1.0
    seed: int = 0
    step0: int = 0
    logit_bias: Union[None, Mapping[int, float], Sequence[Tuple[int, float]]] = None
    allowed_token_ids: Optional[Sequence[int]] = None
    banned_token_ids: Optional[Sequence[int]] = None
    min_new_tokens: int = 0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0

    def __post_init__(self):
        for name in ("presence_penalty", "frequency_penalty"):
            v = float(getattr(self, name))
            if not math.isfinite(v):
                raise ValueError(f"SamplingParams: {name} must be finite, got {v}")
            object.__setattr__(self, name, v)
        bias = self.logit_bias
        bias = tuple((int(i), float(v)) for i, v in (bias.items() if isinstance(bias, Mapping) else (bias or ())))
        for i, v in bias:
            if math.isnan(v) or v == math.inf:
                raise ValueError(f"SamplingParams: logit_bias values are finite or -inf, got {v} for id {i}")
        object.__setattr__(self, "logit_bias", bias)
        if self.allowed_token_ids is not None:
            allowed = tuple(int(i) for i in self.allowed_token_ids)
            if not allowed:
                raise ValueError("SamplingParams: allowed_token_ids is None or a non-empty sequence of ids")
            object.__setattr__(self, "allowed_token_ids", allowed)
        object.__setattr__(self, "banned_token_ids", tuple(int(i) for i in (self.banned_token_ids or ())))
        if int(self.min_new_tokens) < 0:
            raise ValueError(f"SamplingParams: min_new_tokens must be >= 0, got {self.min_new_tokens}")
        if not 0 <= int(self.top_k) <= MAX_TOP_K:
            raise ValueError(f"SamplingParams: top_k must be in [0, {MAX_TOP_K}], got {self.top_k}")
        if not self.temperature > 0.0:
            raise ValueError(f"SamplingParams: temperature must be positive, got {self.temperature}")
        if not self.top_p <= 1.0:
            raise ValueError(f"SamplingParams: top-p should be in (0, 1], got {self.top_p}")
        if not 0.0 <= self.min_p < 1.0:
            raise ValueError(f"SamplingParams: min_p must be in [0, 1), got {self.min_p}")
        if self.min_p > 0.0 and self.top_k != 0:
            raise ValueError("SamplingParams: min_p belongs to the whole-vocabulary branch (top_k == 0)")
        if not self.repetition_penalty > 0.0:
            raise ValueError(f"SamplingParams: repetition_penalty must be positive, got {self.repetition_penalty}")
        if self.step0 < 0:
            raise ValueError(f"SamplingParams: step0 must be >= 0, got {self.step0}")


def _signed64(v: int) -> int:
    v = int(v) & (2 ** 64 - 1)
    return v - 2 ** 64 if v >= 2 ** 63 else v


def pack_rows(params_list: Sequence[SamplingParams], device) -> dict:
    """The setting tensors of sample_rows for a list of SamplingParams, row b from params_list[b]: a dict with top_k (int32), top_p,
    temperature, min_p, penalty (float32), seeds (the uint64 seed's bits in an int64) and steps (int64, step0)."""
    n = len(params_list)
    f = torch.tensor([[p.top_p, p.temperature, p.min_p, p.repetition_penalty] for p in params_list], dtype=torch.float32).reshape(n, 4).t().contiguous()
    i = torch.tensor([[_signed64(p.seed), p.step0] for p in params_list], dtype=torch.int64).reshape(n, 2).t().contiguous()
    k = torch.tensor([p.top_k for p in params_list], dtype=torch.int32)
    f, i, k = f.to(device), i.to(device), k.to(device)
    return {"top_k": k, "top_p": f[0], "temperature": f[1], "min_p": f[2], "penalty": f[3], "seeds": i[0], "steps": i[1]}


def has_count_penalties(p: SamplingParams) -> bool:
    """Whether the request has a presence or a frequency penalty that is not 0."""
    return p.presence_penalty != 0.0 or p.frequency_penalty != 0.0


def pack_count_penalties(params_list: Sequence[SamplingParams], device) -> dict:
    """The penalty tensors of sample_rows / penalty_edits for a list of SamplingParams, row b from params_list[b]: a dict with frequency
    and presence (float32 (n,)).  (pack_rows keeps its keys: callers splat it into sample_rows.)"""
    n = len(params_list)
    f = torch.tensor([[p.frequency_penalty, p.presence_penalty] for p in params_list], dtype=torch.float32).reshape(n, 2).t().contiguous().to(device)
    return {"frequency": f[0], "presence": f[1]}


def has_edits(p: SamplingParams) -> bool:
    """Whether the request's own settings edit its logits (min_new_tokens aside: that is the caller's extra ban)."""
    return bool(p.logit_bias) or p.allowed_token_ids is not None or bool(p.banned_token_ids)


def edit_list(p: SamplingParams, extra_bans: Sequence[int] = ()) -> Tuple[list, int]:
    """The (id, value) entries of one request's edit list and its mode, by the merge rule: extra_bans first with -inf; a banned id -inf; with an
    allowed set the list is the allowed ids, each with its bias or 0 (banned ones -inf; a bias outside the set is dropped), mode 1; without
    one the bias keys and the banned ids, mode 0.  Every id once: its first entry, and of a repeated bias key the first value."""
    bias = {}
    for i, v in p.logit_bias:
        bias.setdefault(i, v)
    banned = set(p.banned_token_ids) | set(extra_bans)
    keys = list(extra_bans) + (list(p.allowed_token_ids) if p.allowed_token_ids is not None else [i for i, _ in p.logit_bias] + list(p.banned_token_ids))
    out, seen = [], set()
    for i in keys:
        if i not in seen:
            seen.add(i)
            out.append((i, -math.inf if i in banned else bias.get(i, 0.0)))
    return out, int(p.allowed_token_ids is not None)


def pack_edits(params_list: Sequence[SamplingParams], device, extra_bans: Optional[Sequence[Sequence[int]]] = None, width: int = 0) -> dict:
    """The edit tensors of sample_rows for a list of SamplingParams, row b from params_list[b] (edit_list): a dict with edit_ids (int64 (n, E)),
    edit_vals (float32 (n, E)), edit_lens and edit_mode (int32 (n,)).  E is the longest list (at least 1, at least `width`); extra_bans[b]:
    ids that go to the front of row b's list with -inf (an allow-only row stays allow-only: a banned id that is not in its set is -inf
    either way)."""
    n = len(params_list)
    lists = [edit_list(p, () if extra_bans is None else extra_bans[b]) for b, p in enumerate(params_list)]
    E = max([1, int(width)] + [len(l) for l, _ in lists])
    ids = torch.zeros(n, E, dtype=torch.int64)
    vals = torch.zeros(n, E, dtype=torch.float32)
    for b, (l, _) in enumerate(lists):
        if l:
            ids[b, :len(l)] = torch.tensor([i for i, _ in l], dtype=torch.int64)
            vals[b, :len(l)] = torch.tensor([v for _, v in l], dtype=torch.float32)
    lens = torch.tensor([len(l) for l, _ in lists], dtype=torch.int32)
    mode = torch.tensor([m for _, m in lists], dtype=torch.int32)
    return {"edit_ids": ids.to(device), "edit_vals": vals.to(device), "edit_lens": lens.to(device), "edit_mode": mode.to(device)}


def apply_logit_edits(logits: torch.Tensor, edit_ids: Optional[torch.Tensor] = None, edit_vals: Optional[torch.Tensor] = None,
                      edit_lens: Optional[torch.Tensor] = None, edit_mode: Optional[torch.Tensor] = None, *, penalty: Optional[torch.Tensor] = None,
                      history: Optional[torch.Tensor] = None, history_lens: Optional[torch.Tensor] = None,
                      frequency: Optional[torch.Tensor] = None, presence: Optional[torch.Tensor] = None,
                      count_start: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The rule of omk_sample_rows (include/omk.h, ABI 14 and 16) in torch, on a copy: the repetition penalty over history[b, :history_lens[b]]
    (rounded to the dtype of the logits), then the edits -- a listed token gets round(float(p) + the value of its FIRST entry), an unlisted
    token of an allow-only row whose list holds a valid id gets -inf.  Lengths are clamped, ids outside [0, vocab) skipped, as the kernel
    does.  What sample_rows draws from when the library declines the fused launch, and the statement the tests check that launch against.
    frequency / presence (float32 (n,), either may be None = 0) with history, history_lens and count_start (int32 (n,), None = 0): the
    presence and frequency penalties of ABI 17 -- a token that occurs c > 0 times in history[b, count_start[b]:history_lens[b]] gets
    delta = -((frequency[b] * c) + presence[b]) (product and sum rounded separately; a non-finite penalty counts as 0): a listed token
    round(float(p) + (value + delta)), an unlisted one round(float(p) + delta) unless the row is allow-only.  All three None: the function
    as it was."""
    n, V = logits.shape
    dev = logits.device
    work = logits
    counted = None
    if frequency is not None or presence is not None:
        if history is None or history_lens is None:
            raise ValueError("apply_logit_edits: frequency / presence need history and history_lens")
        cap = history.shape[1]
        hl = history_lens.long().clamp(0, cap)
        cs = torch.zeros_like(hl) if count_start is None else torch.minimum(count_start.long().clamp(min=0), hl)
        pos = torch.arange(cap, device=dev)[None]
        live = (pos >= cs[:, None]) & (pos < hl[:, None]) & (history >= 0) & (history < V)
        # integer counts; dead entries go to a spare column
        cnt = torch.zeros(n, V + 1, dtype=torch.int64, device=dev).scatter_add_(1, torch.where(live, history, torch.full_like(history, V)),
                                                                                 torch.ones_like(history))[:, :V]
        zero = torch.zeros(n, dtype=torch.float32, device=dev)
        fr = zero if frequency is None else torch.where(torch.isfinite(frequency), frequency.float(), zero)
        pr = zero if presence is None else torch.where(torch.isfinite(presence), presence.float(), zero)
        prod = fr[:, None] * cnt.float()          # (two roundings: the product, then the sum)
        delta = -(prod + pr[:, None])
        counted = cnt > 0
    if penalty is not None and history is not None:
        # a mask of the history ids -- every write is True, so duplicates and the order of the writes do not matter; dead entries go to a
        # spare column
        cap = history.shape[1]
        live = (torch.arange(cap, device=dev)[None] < history_lens[:, None]) & (history >= 0) & (history < V)
        mask = torch.zeros(n, V + 1, dtype=torch.bool, device=dev).scatter_(1, torch.where(live, history, torch.full_like(history, V)), True)[:, :V]
        pen = torch.where(penalty > 0, penalty, torch.ones_like(penalty))[:, None]
        lf = logits.float()
        work = torch.where(mask, torch.where(lf < 0, lf * pen, lf / pen).to(logits.dtype), logits)
    if edit_ids is None or edit_ids.shape[1] == 0:
        if counted is not None:
            return torch.where(counted, (work.float() + delta).to(logits.dtype), work)
        return work.clone() if work is logits else work
    cap = edit_ids.shape[1]
    pos = torch.arange(cap, device=dev)[None].expand(n, cap)
    live = (pos < edit_lens[:, None]) & (edit_ids >= 0) & (edit_ids < V)
    # the first entry of every listed token: the lowest entry index per column (a minimum: the order of the writes does not matter)
    first = torch.full((n, V + 1), cap, dtype=torch.int64, device=dev).scatter_reduce_(
        1, torch.where(live, edit_ids, torch.full_like(edit_ids, V)), pos.contiguous(), "amin")[:, :V]
    listed = first < cap
    add = edit_vals.float().gather(1, first.clamp(max=cap - 1))
    allow = (edit_mode == 1 if edit_mode is not None else torch.zeros(n, dtype=torch.bool, device=dev)) & listed.any(1)
    if counted is None:
        edited = (work.float() + add).to(logits.dtype)
        return torch.where(listed, edited, torch.where(allow[:, None], torch.full_like(work, float("-inf")), work))
    edited = (work.float() + torch.where(counted, add + delta, add)).to(logits.dtype)     # (the inner sum first)
    unlisted = torch.where(counted, (work.float() + delta).to(logits.dtype), work)
    return torch.where(listed, edited, torch.where(allow[:, None], torch.full_like(work, float("-inf")), unlisted))


# ---- guided decoding: per-row token bitmasks (omk_sample_rows_masked; include/omk.h has the rule) ----------------------------------------

def mask_words(vocab: int) -> int:
    """Words of a packed token mask over `vocab` tokens."""
    return (int(vocab) + 31) // 32


def pack_token_mask(allowed_ids, vocab: int) -> torch.Tensor:
    """The packed mask that allows exactly `allowed_ids`: a CPU int32 tensor of (ceil(vocab / 32),), bit (i & 31) of word (i >> 5) set =
    token i may be drawn (the bit order of include/omk.h, and of the masks grammar engines emit).  An id outside [0, vocab): ValueError."""
    import numpy as np
    vocab = int(vocab)
    ids = np.asarray(list(allowed_ids), dtype=np.int64).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() >= vocab):
        raise ValueError(f"pack_token_mask: ids must be in [0, {vocab})")
    bits = np.zeros(mask_words(vocab) * 32, dtype=np.uint8)
    bits[ids] = 1
    return torch.from_numpy(np.packbits(bits, bitorder="little").view("<u4").astype(np.int32))


def apply_token_mask(logits: torch.Tensor, token_mask: torch.Tensor, mask_on: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The mask rule of omk_sample_rows_masked in torch, on a copy: token i of row b keeps its logit when bit (i & 31) of
    token_mask[b, i >> 5] is set or mask_on[b] == 0 (mask_on None: every row is masked), and reads -inf otherwise.  token_mask: int32
    (batch, W >= ceil(vocab / 32)); bits at positions >= vocab are ignored.  What sample_rows draws from when the library declines the
    masked launch, and the statement the tests check that launch against."""
    n, V = logits.shape
    if token_mask.dtype != torch.int32 or token_mask.dim() != 2 or token_mask.shape[0] != n or token_mask.shape[1] < mask_words(V) or token_mask.device != logits.device:
        raise ValueError(f"apply_token_mask: token_mask must be int32 ({n}, >= {mask_words(V)}) on {logits.device}")
    idx = torch.arange(V, device=logits.device)
    keep = ((token_mask[:, idx >> 5] >> (idx & 31)[None]) & 1).bool()
    if mask_on is not None:
        keep = keep | (mask_on == 0)[:, None]
    return torch.where(keep, logits, torch.full_like(logits, float("-inf")))


class ChoiceGuide:
    """A guide that makes its request emit exactly one of `choices` (token-id sequences) and then `eos_token_id`: a walk down the trie of
    the choices.  Where a complete choice is also a proper prefix of another, EOS and the continuation are both allowed.

    The guide protocol (decode_ragged(guides=...); no base class is required) is two methods:
      mask() -> Optional[Tensor]    an int32 (ceil(vocab / 32),) CPU tensor in the bit order of pack_token_mask, or None = unconstrained for
                                    this draw; called once in front of every draw of the guide's request
      advance(token_id: int)        called with every id the request samples, in order, EOS included
    Empty `choices`, an empty sequence, an id outside [0, vocab), or EOS inside a choice: ValueError."""

    def __init__(self, choices, vocab: int, eos_token_id: int):
        self.vocab, self.eos = int(vocab), int(eos_token_id)
        if not 0 <= self.eos < self.vocab:
            raise ValueError(f"ChoiceGuide: eos_token_id must be in [0, {self.vocab})")
        choices = [[int(t) for t in c] for c in choices]
        if not choices:
            raise ValueError("ChoiceGuide: choices is a non-empty list of token-id sequences")
        self.root = {"next": {}, "end": False, "mask": None}
        for c in choices:
            if not c:
                raise ValueError("ChoiceGuide: a choice is a non-empty token-id sequence")
            node = self.root
            for t in c:
                if not 0 <= t < self.vocab or t == self.eos:
                    raise ValueError(f"ChoiceGuide: a choice holds ids in [0, {self.vocab}) other than eos_token_id, got {t}")
                node = node["next"].setdefault(t, {"next": {}, "end": False, "mask": None})
            node["end"] = True
        self.node, self.done = self.root, False
        self._eos_mask = pack_token_mask([self.eos], self.vocab)

    def mask(self) -> torch.Tensor:
        if self.done:
            return self._eos_mask       # (a request that goes on behind its EOS can only repeat it)
        node = self.node
        if node["mask"] is None:
            node["mask"] = pack_token_mask(list(node["next"]) + ([self.eos] if node["end"] else []), self.vocab)
        return node["mask"]

    def advance(self, token_id: int) -> None:
        token_id = int(token_id)
        if self.done:
            return
        if token_id == self.eos and self.node["end"]:
            self.done = True
        elif token_id in self.node["next"]:
            self.node = self.node["next"][token_id]
        else:
            raise ValueError(f"ChoiceGuide: id {token_id} is not one the guide allowed at this point")


def _ptr(t: Optional[torch.Tensor], dtype, n: int, name: str, dev, what: str = "sample_rows"):
    if t is None:
        return None
    if t.dtype != dtype or t.device != dev or t.dim() != 1 or t.shape[0] != n or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be a dense {dtype} tensor of ({n},) on {dev}")
    return t.data_ptr()


PENALTY_MAX_VOCAB = 65536     # tokens the id map of the sampler's edit launch holds (SAMPLE_PEN_MAX_V of sample.hip)


def _rows2d(t, dtype, n, name, dev, what):
    if t.dtype != dtype or t.device != dev or t.dim() != 2 or t.shape[0] != n or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{what}: {name} must be {dtype} (batch, cap) with unit last stride on {dev}")


def penalty_edits(history: torch.Tensor, history_lens: torch.Tensor, count_start: torch.Tensor, frequency: torch.Tensor, presence: torch.Tensor,
                  vocab: int, *, active: Optional[torch.Tensor] = None, edit_ids: Optional[torch.Tensor] = None, edit_vals: Optional[torch.Tensor] = None,
                  edit_lens: Optional[torch.Tensor] = None, edit_mode: Optional[torch.Tensor] = None, out: Optional[dict] = None,
                  out_cap: Optional[int] = None) -> dict:
    """ONE launch (omk_penalty_edits, ABI 17; include/omk.h has the rule): per row the edit list that makes omk_sample_rows apply the presence
    and frequency penalties over history[b, count_start[b]:history_lens[b]] -- the row's user entries (edit_ids / edit_vals / edit_lens /
    edit_mode, optional, the layouts of sample_rows) with the delta of a counted id added to its value, then (id, delta) for every other
    distinct counted token in the order of first occurrence.  Returns a dict edit_ids (int64 (n, cap)), edit_vals (float32), edit_lens,
    edit_mode (int32 (n,)) to splat into sample_rows.  out: such a dict of caller-owned buffers (they must not be the user list); otherwise
    they are allocated out_cap wide (default: user width + history width, at least 1; what does not fit is dropped; the lengths and modes
    are zero-filled, two small fill launches, the ids and values are not initialised behind a row's length).  No host read:
    capturable, every tensor may be rewritten between replays."""
    lib = get_lib()
    what = "penalty_edits"
    n, dev = history.shape[0], history.device
    _rows2d(history, torch.int64, n, "history", dev, what)
    p = K.PenaltyEdits(history=history.data_ptr(), history_stride=history.stride(0), history_cap=history.shape[1],
                       history_lens=_ptr(history_lens, torch.int32, n, "history_lens", dev, what), count_start=_ptr(count_start, torch.int32, n, "count_start", dev, what),
                       frequency=_ptr(frequency, torch.float32, n, "frequency", dev, what), presence=_ptr(presence, torch.float32, n, "presence", dev, what),
                       active=_ptr(active, torch.int32, n, "active", dev, what), batch=n, vocab=int(vocab))
    width = 0
    if edit_ids is not None:
        _rows2d(edit_ids, torch.int64, n, "edit_ids", dev, what)
        if edit_vals is not None and (edit_vals.dtype != torch.float32 or edit_vals.device != dev or edit_vals.shape != edit_ids.shape or edit_vals.stride() != edit_ids.stride()):
            raise ValueError("penalty_edits: edit_vals must be float32 with the shape and strides of edit_ids on the device of history")
        width = edit_ids.shape[1]
        p.edit_ids, p.edit_stride, p.edit_cap = edit_ids.data_ptr(), edit_ids.stride(0), width
        p.edit_vals = None if edit_vals is None else edit_vals.data_ptr()
        p.edit_lens, p.edit_mode = _ptr(edit_lens, torch.int32, n, "edit_lens", dev, what), _ptr(edit_mode, torch.int32, n, "edit_mode", dev, what)
    if out is None:
        cap = max(1, width + history.shape[1]) if out_cap is None else int(out_cap)
        # (entries behind a row's length are never read: the two wide buffers are left as allocated)
        out = {"edit_ids": torch.empty(n, cap, dtype=torch.int64, device=dev), "edit_vals": torch.empty(n, cap, dtype=torch.float32, device=dev),
               "edit_lens": torch.zeros(n, dtype=torch.int32, device=dev), "edit_mode": torch.zeros(n, dtype=torch.int32, device=dev)}
    oi, ov = out["edit_ids"], out["edit_vals"]
    _rows2d(oi, torch.int64, n, "out edit_ids", dev, what)
    if ov.dtype != torch.float32 or ov.device != dev or ov.shape != oi.shape or ov.stride() != oi.stride():
        raise ValueError("penalty_edits: out edit_vals must be float32 with the shape and strides of out edit_ids")
    if edit_ids is not None and (oi.data_ptr() == edit_ids.data_ptr() or (edit_vals is not None and ov.data_ptr() == edit_vals.data_ptr())):
        raise ValueError("penalty_edits: the output buffers must not be the user list")
    p.out_ids, p.out_vals, p.out_stride, p.out_cap = oi.data_ptr(), ov.data_ptr(), oi.stride(0), oi.shape[1]
    p.out_lens, p.out_mode = _ptr(out["edit_lens"], torch.int32, n, "out edit_lens", dev, what), _ptr(out["edit_mode"], torch.int32, n, "out edit_mode", dev, what)
    if n > 0 and (p.out_ids is None or p.history is None):      # (an empty tensor has no data pointer: a zero-width history or output)
        raise ValueError("penalty_edits: history and the output buffers must be at least one entry wide")
    K.run(lib, "omk_penalty_edits", p, history)
    return out


def sample_rows(logits: torch.Tensor, *, top_k: Optional[torch.Tensor], top_p: Optional[torch.Tensor], temperature: Optional[torch.Tensor],
                min_p: Optional[torch.Tensor], seeds: Optional[torch.Tensor], steps: Optional[torch.Tensor], penalty: Optional[torch.Tensor] = None,
                history: Optional[torch.Tensor] = None, history_lens: Optional[torch.Tensor] = None, active: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, edit_ids: Optional[torch.Tensor] = None, edit_vals: Optional[torch.Tensor] = None,
                edit_lens: Optional[torch.Tensor] = None, edit_mode: Optional[torch.Tensor] = None, frequency: Optional[torch.Tensor] = None,
                presence: Optional[torch.Tensor] = None, count_start: Optional[torch.Tensor] = None, count_max: Optional[int] = None,
                merged: Optional[dict] = None, token_mask: Optional[torch.Tensor] = None, mask_on: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(batch, vocab) -> (batch,) int64 ids in ONE launch, row b sampled with its own settings: top_k (int32), top_p, temperature, min_p
    (float32), seeds and steps (int64; the seed's 64 bits) -- device tensors of (batch,).  Row b draws what
    sample_device(logits[b:b+1], ..., seed=seeds[b], offset=steps[b]) draws: its id does not depend on its place in the batch.
    penalty (float32) with history (int64 (batch, cap), unit last stride) and history_lens (int32): the repetition penalty of
    generation.modify_logit_for_repetition_penalty over history[b, :history_lens[b]], fused (logits is not written).  active (int32):
    rows with 0 write nothing.  edit_ids (int64 (batch, cap), unit last stride) with edit_vals (float32, the same shape and strides) and
    edit_lens (int32), optionally edit_mode (int32): per-row logit edits behind the penalty, fused (pack_edits makes them, apply_logit_edits
    states the rule).  No host read: capturable, the tensors may be rewritten between replays.  A vocabulary too large for the kernel's id
    map, or more than MAX_EDITS entries per row: the penalty and the edits are applied to a copy with torch and the plain launch draws.
    frequency / presence (float32, either may be None = 0) with history, history_lens and count_start (int32, None = 0): the presence and
    frequency penalties over history[b, count_start[b]:history_lens[b]] (apply_logit_edits states the rule).  count_max: the host-known upper
    bound of the rows' counted lengths (default: the width of history).  It is taken on trust -- the launch cannot check it: if a row
    counts more distinct tokens than count_max, the merged list is cut at edit width + count_max entries and the tokens that do not fit
    get NO penalty.  With a vocabulary of at most PENALTY_MAX_VOCAB tokens and
    edit width + count_max <= MAX_EDITS: TWO kernels of the library and no host read (with `merged` nothing else; without it the buffers
    are allocated and their lengths zero-filled first) -- penalty_edits builds the rows' merged lists (into `merged`, a dict
    of caller-owned static buffers as penalty_edits returns it, at least edit width + count_max and at most MAX_EDITS wide; allocated when
    None), then the edit launch draws.  Otherwise a copy is edited with apply_logit_edits and the plain launch draws.  Both None: the
    function as it was.
    token_mask (int32 (batch, W >= ceil(vocab / 32)), unit last stride, on the device of logits; pack_token_mask gives a row) with mask_on
    (int32 (batch,), optional: 0 = the row ignores its mask): guided decoding -- a token whose bit is clear is never drawn, applied LAST,
    behind the penalties and the edits, inside the launch (omk_sample_rows_masked; apply_token_mask states the rule).  With frequency /
    presence: penalty_edits first, then the masked launch.  Where the library declines (a vocabulary above PENALTY_MAX_VOCAB, more than
    MAX_EDITS entries), the mask is applied to the copy as well and the plain launch draws.  token_mask None: the function as it was,
    through omk_sample_rows."""
    if token_mask is None and mask_on is not None:
        raise ValueError("sample_rows: mask_on needs token_mask")
    if frequency is not None or presence is not None:
        return _rows_count_penalties(logits, dict(top_k=top_k, top_p=top_p, temperature=temperature, min_p=min_p, seeds=seeds, steps=steps, active=active, out=out),
                                     dict(penalty=penalty, history=history, history_lens=history_lens),
                                     dict(edit_ids=edit_ids, edit_vals=edit_vals, edit_lens=edit_lens, edit_mode=edit_mode),
                                     frequency, presence, count_start, count_max, merged,
                                     {} if token_mask is None else dict(token_mask=token_mask, mask_on=mask_on))
    p, out = _rows_call(logits, top_k=top_k, top_p=top_p, temperature=temperature, min_p=min_p, seeds=seeds, steps=steps, penalty=penalty, history=history,
                   history_lens=history_lens, active=active, out=out, edit_ids=edit_ids, edit_vals=edit_vals, edit_lens=edit_lens, edit_mode=edit_mode)
    lib = get_lib()
    if token_mask is not None:
        if K.try_run(lib, "omk_sample_rows_masked", _masked_call(p, logits, token_mask, mask_on), logits):
            return out
    elif K.try_run(lib, "omk_sample_rows", p, logits):
        return out
    work = apply_logit_edits(logits, edit_ids, edit_vals, edit_lens, edit_mode, penalty=penalty, history=history, history_lens=history_lens)
    if token_mask is not None:
        work = apply_token_mask(work, token_mask, mask_on)
    p.logits = K.T(work)
    p.penalty = p.history = p.history_lens = p.edit_ids = p.edit_vals = p.edit_lens = p.edit_mode = None
    p.edit_cap = 0
    K.run(lib, "omk_sample_rows", p, logits)
    return out


def _rows_count_penalties(logits, base, rep, user, frequency, presence, count_start, count_max, merged, guide):
    """sample_rows with a presence / frequency penalty: penalty_edits + the edit launch, or the plain launch on an edited copy."""
    n, dev = logits.shape[0], logits.device
    history, history_lens = rep["history"], rep["history_lens"]
    if history is None or history_lens is None:
        raise ValueError("sample_rows: frequency / presence need history and history_lens")
    zero = None
    if frequency is None or presence is None or count_start is None:
        zero = torch.zeros(n, dtype=torch.float32, device=dev)
    frequency = zero if frequency is None else frequency
    presence = zero if presence is None else presence
    count_start = zero.int() if count_start is None else count_start
    count_max = history.shape[1] if count_max is None else int(count_max)
    if count_max < 0:
        raise ValueError(f"sample_rows: count_max must be >= 0, got {count_max}")
    width = 0 if user["edit_ids"] is None else user["edit_ids"].shape[1]
    need = width + count_max
    if merged is not None and not need <= merged["edit_ids"].shape[1]:
        raise ValueError(f"sample_rows: the merged buffers hold {merged['edit_ids'].shape[1]} entries a row, edit width + count_max is {need}")
    cap = max(1, need) if merged is None else merged["edit_ids"].shape[1]
    if n > 0 and history.shape[1] > 0 and logits.shape[1] <= PENALTY_MAX_VOCAB and need <= MAX_EDITS and cap <= MAX_EDITS:
        ed = penalty_edits(history, history_lens, count_start, frequency, presence, logits.shape[1], active=base["active"],
                           **(user if width else {}), out=merged, out_cap=cap)
        return sample_rows(logits, **base, **rep, **ed, **guide)
    work = apply_logit_edits(logits, **user, **rep, frequency=frequency, presence=presence, count_start=count_start)
    if guide:
        work = apply_token_mask(work, **guide)
    return sample_rows(work, **base)


def sample_rows_form(logits: torch.Tensor, **kw) -> int:
    """Which launch sample_rows(logits, **kw) takes -- K.SAMPLE_ROWS_PLAIN / _PENALTY / _EDIT, with a token_mask K.SAMPLE_ROWS_MASK /
    _EDIT_MASK, or the negative omk_status the library refuses the call with.  The launch's own decision (omk_sample_rows_form /
    omk_sample_rows_masked_form); nothing is launched."""
    import ctypes
    token_mask, mask_on = kw.pop("token_mask", None), kw.pop("mask_on", None)
    p = _rows_call(logits, **kw)[0]
    if token_mask is None:
        return int(get_lib().omk_sample_rows_form(ctypes.byref(p)))
    return int(get_lib().omk_sample_rows_masked_form(ctypes.byref(_masked_call(p, logits, token_mask, mask_on))))


def _masked_call(p, logits, token_mask, mask_on):
    """(the OmkSampleRowsMasked around the OmkSampleRows `p` of a sample_rows call; the width of the mask is the library's to check)"""
    n, dev = logits.shape[0], logits.device
    if token_mask.dtype != torch.int32 or token_mask.device != dev or token_mask.dim() != 2 or token_mask.shape[0] != n or (token_mask.shape[1] > 1 and token_mask.stride(1) != 1):
        raise ValueError("sample_rows: token_mask must be int32 (batch, words) with unit last stride on the device of logits")
    return K.SampleRowsMasked(rows=p, mask=token_mask.data_ptr(), mask_on=_ptr(mask_on, torch.int32, n, "mask_on", dev),
                              mask_stride=token_mask.stride(0), mask_words=token_mask.shape[1])


def _rows_call(logits, *, top_k, top_p, temperature, min_p, seeds, steps, penalty=None, history=None, history_lens=None, active=None, out=None,
               edit_ids=None, edit_vals=None, edit_lens=None, edit_mode=None):
    """(the OmkSampleRows of a sample_rows call, its output tensor)"""
    n, dev = logits.shape[0], logits.device
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=dev)
    if out.dtype != torch.int64 or out.device != dev or out.dim() != 1 or out.shape[0] != n:
        raise ValueError("sample_rows: out must be int64 (batch,) on the device of logits")
    p = K.SampleRows(logits=K.T(logits), top_k=_ptr(top_k, torch.int32, n, "top_k", dev), top_p=_ptr(top_p, torch.float32, n, "top_p", dev),
                     temperature=_ptr(temperature, torch.float32, n, "temperature", dev), min_p=_ptr(min_p, torch.float32, n, "min_p", dev),
                     seeds=_ptr(seeds, torch.int64, n, "seeds", dev), steps=_ptr(steps, torch.int64, n, "steps", dev),
                     penalty=_ptr(penalty, torch.float32, n, "penalty", dev), history_lens=_ptr(history_lens, torch.int32, n, "history_lens", dev),
                     active=_ptr(active, torch.int32, n, "active", dev))
    if history is not None:
        if history.dtype != torch.int64 or history.device != dev or history.dim() != 2 or history.shape[0] != n or (history.shape[1] > 1 and history.stride(1) != 1):
            raise ValueError("sample_rows: history must be int64 (batch, cap) with unit last stride on the device of logits")
        p.history, p.history_stride, p.history_cap = history.data_ptr(), history.stride(0), history.shape[1]
    if edit_ids is not None:
        if edit_ids.dtype != torch.int64 or edit_ids.device != dev or edit_ids.dim() != 2 or edit_ids.shape[0] != n or (edit_ids.shape[1] > 1 and edit_ids.stride(1) != 1):
            raise ValueError("sample_rows: edit_ids must be int64 (batch, cap) with unit last stride on the device of logits")
        if edit_vals is not None and (edit_vals.dtype != torch.float32 or edit_vals.device != dev or edit_vals.shape != edit_ids.shape or edit_vals.stride() != edit_ids.stride()):
            raise ValueError("sample_rows: edit_vals must be float32 with the shape and strides of edit_ids on the device of logits")
        p.edit_ids, p.edit_stride, p.edit_cap = edit_ids.data_ptr(), edit_ids.stride(0), edit_ids.shape[1]
        p.edit_vals = None if edit_vals is None else edit_vals.data_ptr()
        p.edit_lens, p.edit_mode = _ptr(edit_lens, torch.int32, n, "edit_lens", dev), _ptr(edit_mode, torch.int32, n, "edit_mode", dev)
    p.out_ids.data = out.data_ptr()
    p.out_ids.ndim = 1
    p.out_ids.shape[0] = n
    p.out_ids.stride[0] = out.stride(0)
    return p, out


# ---- log-probabilities behind the sampler (omk_token_logprobs, ABI 15) ------------------------------------------------------------------

MAX_TOP_N = 64


@dataclass
class TokenLogprobs:
    """What token_logprobs returns; a field that was not asked for is None.  logprob (rows,) float32 and rank (rows,) int32: of the given
    ids; top_ids (rows, top_n) int64 and top_logprobs (rows, top_n) float32: the top_n most likely tokens of every row."""
    logprob: Optional[torch.Tensor] = None
    rank: Optional[torch.Tensor] = None
    top_ids: Optional[torch.Tensor] = None
    top_logprobs: Optional[torch.Tensor] = None


def _desc(t: torch.Tensor) -> K.OmkTensor:
    """Descriptor of an int64 tensor (the C side knows what it points to: its dtype field is not read)."""
    o = K.OmkTensor()
    n = t.dim()
    o.data, o.ndim = t.data_ptr(), n
    o.shape[:n] = t.shape
    o.stride[:n] = t.stride()
    return o


def token_logprobs(logits: torch.Tensor, ids: Optional[torch.Tensor] = None, *, top_n: int = 0, active: Optional[torch.Tensor] = None,
                   out: Optional[TokenLogprobs] = None) -> TokenLogprobs:
    """(rows, vocab) logits -> the log-probabilities of the RAW rows (no temperature, filter or penalty) in ONE launch:
    ids (int64 (rows,)) given: logprob[b] = log_softmax(logits[b])[ids[b]] and rank[b], the 1-based position of ids[b] among the row's
    tokens ordered by (value descending, index ascending); an id outside [0, vocab) gives NaN and rank 0.  top_n in [1, 64]: top_ids and
    top_logprobs, the first top_n tokens of that order (entries past vocab: id -1, -inf).  active (int32 (rows,)): rows with 0 write
    nothing.  out: a TokenLogprobs of buffers to write into (any strides; fields left None are allocated) -- the static buffers of a
    captured launch.  A row's outputs do not depend on its place in the batch.  No host read: capturable, and logits, ids and active may be
    rewritten between replays."""
    lib = get_lib()
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("token_logprobs: logits must be (rows, vocab) with unit last stride")
    n, dev = logits.shape[0], logits.device
    top_n = int(top_n)
    if not 0 <= top_n <= MAX_TOP_N:
        raise ValueError(f"token_logprobs: top_n must be in [0, {MAX_TOP_N}], got {top_n}")
    if ids is None and top_n == 0:
        raise ValueError("token_logprobs: nothing to do: give ids, top_n > 0 or both")
    o = out if out is not None else TokenLogprobs()
    res = TokenLogprobs()

    def buf(t, shape, dtype, name):
        if t is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        if t.dtype != dtype or t.device != dev or tuple(t.shape) != shape:
            raise ValueError(f"token_logprobs: out.{name} must be a {dtype} tensor of {shape} on {dev}")
        return t

    p = K.TokenLogprobs(logits=K.T(logits), top_n=top_n, ids=_ptr(ids, torch.int64, n, "ids", dev, "token_logprobs"),
                        active=_ptr(active, torch.int32, n, "active", dev, "token_logprobs"))
    if ids is not None:
        res.logprob = buf(o.logprob, (n,), torch.float32, "logprob")
        res.rank = buf(o.rank, (n,), torch.int32, "rank")
        p.logprob, p.rank = K.T(res.logprob), K.T(res.rank)
    if top_n > 0:
        res.top_ids = buf(o.top_ids, (n, top_n), torch.int64, "top_ids")
        res.top_logprobs = buf(o.top_logprobs, (n, top_n), torch.float32, "top_logprobs")
        p.top_ids, p.top_logprobs = _desc(res.top_ids), K.T(res.top_logprobs)
    if n > 0:               # (an empty tensor has no data pointer to describe)
        K.run(lib, "omk_token_logprobs", p, logits)
    return res
