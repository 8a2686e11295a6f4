"""Turn-by-turn records of `Segment.track_turns`: the result class, the definition of a record (shared by the fused kernel's
sums and the general path's torch restatement) and the planner that splits the turns into launches."""
from __future__ import annotations

from collections import namedtuple

import torch

#: what `TurnByTurn.tunes` returns: both (..., record_first, len(planes)) float64
Tunes = namedtuple("Tunes", ["tune", "amplitude"])
#: what `TurnByTurn.tune_diffusion` returns: the `Tunes` of the two halves and d (..., record_first) float64
TuneDiffusion = namedtuple("TuneDiffusion", ["first", "second", "d"])

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
    Every tensor lives on the beam's device; nothing here was synchronised with the host.

    From the recorded rows (record_first > 0):
    tunes(planes, first_record, num_records)   `Tunes(tune, amplitude)`, both (..., record_first, len(planes)) float64: per row
                and plane the interpolated peak of the Hann-windowed spectrum of a window of 8 .. 4096 consecutive records (NAFF's
                first line, converging like T^-3 or better in the window length T where an FFT bin resolves 1 / T) and the
                amplitude of that line in the units of the coordinate. The tune is in cycles per RECORD step and lies in
                [0, 1/2]: with record_every = m it is m times the turn tune, folded into [0, 1/2] (q -> |q - round(q)|); it is
                not unfolded. NaN for a row lost up to the window's last record, for a window with a non-finite sample, and
                (amplitude 0) for a constant signal
    tune_diffusion(planes)   `TuneDiffusion(first, second, d)`: the tunes of the first and the second half of the records and
                d = log10 sqrt(sum over planes (tune_2 - tune_1)^2), the frequency-map measure of chaos (-inf where the halves
                agree exactly, NaN where either half is NaN)"""

    __slots__ = ("outgoing", "lost_turn", "turns", "sums", "particles", "_record_every")

    def __init__(self, outgoing, lost_turn: torch.Tensor, turns: torch.Tensor, sums: torch.Tensor, particles=None,
                 record_every=None) -> None:
        assert sums.dim() >= 2 and sums.shape[-1] == NUM_SUMS and sums.dtype == torch.float64 and turns.shape == sums.shape[:1]
        self.outgoing = outgoing
        self.lost_turn = lost_turn
        self.turns = turns
        self.sums = sums
        self.particles = particles
        self._record_every = record_every      # known to the host by `Segment.track_turns`; else read from `turns` when needed

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

    def tunes(self, planes=("x", "y"), first_record: int = 0, num_records=None) -> Tunes:
        """Per recorded row and plane ("x", "y", "tau") the tune and the amplitude of the strongest line of the records
        first_record .. first_record + num_records - 1 (`num_records=None`: every record from `first_record` on); see the class.
        One HIP call (`chx_tunes`), float64 results, bitwise reproducible, no host synchronisation; not differentiable
        (`Segment.track_turns` is not)."""
        from .. import _ops

        if self.particles is None:
            raise ValueError("tunes need the recorded rows: call Segment.track_turns with record_first > 0")
        planes = (planes,) if isinstance(planes, str) else tuple(planes)
        if not planes or any(p not in _ops.TUNES_PLANES for p in planes) or len(set(planes)) != len(planes):
            raise ValueError(f"planes must be distinct names out of {tuple(_ops.TUNES_PLANES)}, got {planes!r}")
        R = int(self.particles.shape[0])
        first_record = int(first_record)
        num_records = R - first_record if num_records is None else int(num_records)
        if not _ops.TUNES_T_MIN <= num_records <= _ops.TUNES_T_MAX:
            raise ValueError(f"a window of {num_records} records: tunes take {_ops.TUNES_T_MIN} to {_ops.TUNES_T_MAX} records. Record "
                             "more turns, thin a long run with record_every, or take windows of it with first_record / num_records")
        if first_record < 0 or first_record + num_records > R:
            raise ValueError(f"records {first_record} .. {first_record + num_records - 1} lie outside the {R} records")
        if self._record_every is None:
            self._record_every = int(self.turns[0])
        K = int(self.particles.shape[-2])
        lead = tuple(self.particles.shape[1:-2])
        probe = self.particles.reshape(R, -1, 7)
        lost = self.lost_turn[..., :K].expand(*lead, K).reshape(-1)
        columns = sum(1 << _ops.TUNES_PLANES[p] for p in planes)
        nu, amp = _ops.tunes(probe, lost, first_record, num_records, (first_record + num_records) * self._record_every, columns)
        order = [sorted(planes, key=_ops.TUNES_PLANES.get).index(p) for p in planes]
        if order != list(range(len(planes))):                      # (column views: no index tensor crosses from the host)
            nu, amp = torch.stack([nu[:, i] for i in order], dim=1), torch.stack([amp[:, i] for i in order], dim=1)
        return Tunes(nu.reshape(*lead, K, len(planes)), amp.reshape(*lead, K, len(planes)))

    def tune_diffusion(self, planes=("x", "y")) -> TuneDiffusion:
        """The tunes of the records [0, T) and [T, 2 T), T = R // 2, and d = log10 sqrt(sum over planes (tune_2 - tune_1)^2):
        -inf where the two halves agree exactly, NaN where either is NaN (a particle lost during the run)."""
        T = (0 if self.particles is None else int(self.particles.shape[0])) // 2
        first = self.tunes(planes, 0, T)
        second = self.tunes(planes, T, T)
        diff = second.tune - first.tune
        return TuneDiffusion(first, second, torch.log10(torch.sqrt((diff * diff).sum(dim=-1))))

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
