"""Turn-by-turn records of `Segment.track_turns`: the result class, the definition of a record (shared by the fused kernel's
sums and the general path's torch restatement) and the planner that splits the turns into launches."""
from __future__ import annotations

import torch

#: sums of one recorded turn, all float64, over the particles alive at the end of that turn: the count, sum w, sum w x_j (j < 6),
#: sum w x_j^2 (j < 6); w = float64(charge) * float64(survival probability of the incoming beam)
NUM_SUMS = 14

#: what one launch of the fused turn kernel does at most: item steps (turns x items; at the ~1-2 us the kernel takes per item step
#: at 1e6 particles about 0.1 s) and bytes of per-workgroup partial sums. `Segment.track_turns` reads them at every call
_MAX_ITEM_STEPS = 65536
_MAX_PARTIAL_BYTES = 64 << 20


class TurnByTurn:
    """What `Segment.track_turns` returns.

    outgoing    the `ParticleBeam` after the last turn. A lost particle stands where it was lost (its coordinates at the end of
                the turn of its loss) and its survival probability is multiplied by 0
    lost_turn   (N,) int32: 0 = alive after the last turn, else the 1-based turn at whose end the particle was lost — one of its
                six coordinates non-finite, or |x| > aperture[0], or |y| > aperture[1]
    turns       (R,) int64: the recorded turn numbers record_every, 2 record_every, ...; R = num_turns // record_every
    num_alive   (R,) float64: particles alive at the end of the recorded turn
    charge      (R,) float64: sum of w over them, w = float64(charge) * float64(survival probability of the incoming beam)
    mean        (R, 6) float64: sum w x_j / sum w (NaN, like std, for a record without live charge: 0 / 0)
    std         (R, 6) float64: sqrt(max(0, sum w x_j^2 / sum w - mean^2)) — the POPULATION form of the weighted spread (divisor
                sum w). `ParticleBeam.sigma_x` and its siblings use the reference's unbiased weighted estimator instead; the two
                differ by a factor close to sqrt(1 - 1 / N)
    sums        (R, 14) float64: the raw sums behind the four fields above (count, sum w, sum w x_j, sum w x_j^2)
    particles   (R, record_first, 7) in the beam's dtype: rows 0 .. record_first - 1 of the beam at the recorded turns (a lost row
                with its frozen values), or None when record_first = 0

    A vectorised beam or lattice (the general path) puts its batch dimensions behind R and in front of N: lost_turn (..., N),
    num_alive (R, ...), mean (R, ..., 6), particles (R, ..., record_first, 7).
    Every tensor lives on the beam's device; nothing here was synchronised with the host."""

    __slots__ = ("outgoing", "lost_turn", "turns", "sums", "particles")

    def __init__(self, outgoing, lost_turn: torch.Tensor, turns: torch.Tensor, sums: torch.Tensor, particles=None) -> None:
        assert sums.dim() >= 2 and sums.shape[-1] == NUM_SUMS and sums.dtype == torch.float64 and turns.shape == sums.shape[:1]
        self.outgoing = outgoing
        self.lost_turn = lost_turn
        self.turns = turns
        self.sums = sums
        self.particles = particles

    @property
    def num_alive(self) -> torch.Tensor:
        return self.sums[..., 0]

    @property
    def charge(self) -> torch.Tensor:
        return self.sums[..., 1]

    @property
    def mean(self) -> torch.Tensor:
        return self.sums[..., 2:8] / self.sums[..., 1:2]

    @property
    def std(self) -> torch.Tensor:
        mean = self.mean
        return torch.sqrt(torch.clamp(self.sums[..., 8:14] / self.sums[..., 1:2] - mean * mean, min=0.0))

    def __repr__(self) -> str:
        return f"TurnByTurn(records={self.turns.shape[0]}, particles={tuple(self.lost_turn.shape)})"


def recorded_turns(num_turns: int, record_every: int, device=None) -> torch.Tensor:
    """(R,) int64: the recorded turn numbers of a call, every multiple of `record_every` up to `num_turns`."""
    return torch.arange(1, num_turns // record_every + 1, dtype=torch.int64, device=device) * record_every


def plan_chunks(num_turns: int, items: int, record_every: int, partial_bytes_per_record: int, max_item_steps: int,
                max_partial_bytes: int) -> list:
    """[(first_turn, turns)]: the launches of a fused call. The ranges cover the turns 1 .. num_turns once and in order. A launch
    does at most `max_item_steps` item steps (turns x items) and records at most `max_partial_bytes // partial_bytes_per_record`
    turns — but never less than one whole turn and one record: a turn is not split. Which turns are recorded does not depend on
    the split (turn t is recorded when t % record_every == 0, wherever the chunk around it begins)."""
    if num_turns < 1 or items < 1 or record_every < 1:
        raise ValueError("num_turns, items and record_every must be at least 1")
    by_steps = max(1, max_item_steps // items)
    by_records = max(1, max_partial_bytes // max(1, partial_bytes_per_record)) * record_every   # k record_every turns hold k records
    per_launch = min(by_steps, by_records, num_turns)
    return [(first, min(per_launch, num_turns - first + 1)) for first in range(1, num_turns + 1, per_launch)]


def chunk_records(first_turn: int, turns: int, record_every: int) -> int:
    """Recorded turns within [first_turn, first_turn + turns)."""
    return (first_turn + turns - 1) // record_every - (first_turn - 1) // record_every


def is_lost(x: torch.Tensor, aperture) -> torch.Tensor:
    """(..., N) bool: the loss rule on the rows of x (..., N, 7) — a non-finite coordinate among the six, or outside the aperture."""
    bad = ~torch.isfinite(x[..., :6]).all(dim=-1)
    if aperture is not None:
        bad = bad | (x[..., 0].abs() > aperture[0]) | (x[..., 2].abs() > aperture[1])
    return bad


def record_sums(x: torch.Tensor, alive: torch.Tensor, w) -> torch.Tensor:
    """(..., 14) float64: the sums of one record over the rows of x (..., N, 7) with `alive` (..., N) bool and the weights w
    (..., N) float64 or None, restated with torch operations — the general path of `Segment.track_turns`; leading dimensions
    are the beams of a vectorised beam. Rows that are not alive are SELECTED out (a NaN times 0 would stay a NaN)."""
    xd = x[..., :6].to(torch.float64)
    wd = torch.ones(x.shape[-2], dtype=torch.float64, device=x.device) if w is None else w
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    alive, wd = torch.broadcast_tensors(alive, wd)
    live = alive.unsqueeze(-1)
    wx = wd.unsqueeze(-1) * xd
    return torch.cat([alive.sum(dim=-1, dtype=torch.float64).unsqueeze(-1), torch.where(alive, wd, zero).sum(dim=-1).unsqueeze(-1),
                      torch.where(live, wx, zero).sum(dim=-2), torch.where(live, wx * xd, zero).sum(dim=-2)], dim=-1)
