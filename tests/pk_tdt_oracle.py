"""Oracle of Parakeet's TDT decoder (crispy_pk_tdt_*, include/crispy_hip.h): the encoder projector, the LSTM prediction network and
the joint head as torch modules whose attribute names give the state-dict keys of transformers' ParakeetForTDT, constructible in
float32 and float64, and the greedy loop on one clip at a time.  tests/test_pk_tdt_oracle.py pins this file on
transformers.models.parakeet (where present) and on tests/golden/parakeet_tdt_golden.npz.

The loop on frames e[0 .. T'): p = encoder_projector(e); (h, c) = 0, g = decoder_projector(lstm(embedding[blank])); at each step
logits = head(relu(p[t] + g)), k = arg-max of the first V, d = durations[arg-max of the last n_d], a blank with d == 0 takes d = 1,
the step (k, t, d) is recorded and t += d; a non-blank k runs the prediction network on embedding[k] and replaces (h, c, g).  It ends
with t >= T' or after max_symbols_per_step * T' - 1 steps."""
import math
from dataclasses import dataclass

import numpy as np
import torch
from torch import nn

from tests import pk_oracle as PO

MARK = "▁"      # the piece prefix that starts a word


@dataclass(frozen=True)
class TdtConfig:
    hidden: int
    decoder_hidden: int
    decoder_layers: int
    vocab: int
    blank: int
    durations: tuple = (0, 1, 2, 3, 4)
    max_symbols_per_step: int = 10

    @property
    def n_durations(self):
        return len(self.durations)

    @property
    def width(self):
        return self.vocab + len(self.durations)

    def as_dict(self):
        """the fields of crispy_pk_tdt_config"""
        return dict(hidden=self.hidden, decoder_hidden=self.decoder_hidden, decoder_layers=self.decoder_layers, vocab=self.vocab,
                    blank=self.blank, n_durations=len(self.durations), durations=list(self.durations) + [0] * (8 - len(self.durations)),
                    max_symbols_per_step=self.max_symbols_per_step)


TINY_TDT = TdtConfig(hidden=PO.TINY.hidden, decoder_hidden=128, decoder_layers=2, vocab=33, blank=32)
CATALOG_TDT = TdtConfig(hidden=1024, decoder_hidden=640, decoder_layers=2, vocab=8193, blank=8192)


def max_steps(cfg: TdtConfig, frames: int) -> int:
    """the step budget of one clip: generate()'s max_length = max_symbols_per_step * T' counts the start token"""
    return max(0, cfg.max_symbols_per_step * frames - 1) if frames > 0 else 0


def frames(t: int, hidden: int, seed: int, scale: float = 1.0) -> np.ndarray:
    """seeded encoder frames f32 [t][hidden]"""
    return (np.random.default_rng(seed).standard_normal((t, hidden)) * scale).astype(np.float32)


class Decoder(nn.Module):
    def __init__(self, c: TdtConfig):
        super().__init__()
        self.embedding = nn.Embedding(c.vocab, c.decoder_hidden)
        self.lstm = nn.LSTM(input_size=c.decoder_hidden, hidden_size=c.decoder_hidden, num_layers=c.decoder_layers, batch_first=True)
        self.decoder_projector = nn.Linear(c.decoder_hidden, c.decoder_hidden)


class Joint(nn.Module):
    def __init__(self, c: TdtConfig):
        super().__init__()
        self.head = nn.Linear(c.decoder_hidden, c.vocab + len(c.durations))


class TdtModules(nn.Module):
    def __init__(self, c: TdtConfig):
        super().__init__()
        self.encoder_projector = nn.Linear(c.hidden, c.decoder_hidden)
        self.decoder = Decoder(c)
        self.joint = Joint(c)


def tensor_list(c: TdtConfig):
    """(key, element count) in state-dict order"""
    return [(k, int(v.numel())) for k, v in TdtModules(c).state_dict().items()]


# Weight sets of the tests.  Random matrices at 1 / sqrt(fan-in) with small biases decode degenerately (every duration the same, no
# blank), so the head and the two projectors are scaled up until the frame and the state both move the arg-max, and the blank and
# duration biases choose the mix: MIX has every duration and blanks beside tokens, STALL prefers tokens of duration 0 (its clips
# stay at one frame and end on the step budget), BLANKS emits nothing but blanks, TOKENS never a blank.
MIX = dict(blank_bias=4.0, duration_bias=(-4.0, 0.5, 0.0, 0.0, 0.0))
STALL = dict(blank_bias=-30.0, duration_bias=(30.0, 0.0, 0.0, 0.0, 0.0))
BLANKS = dict(blank_bias=60.0, duration_bias=(0.0, 0.0, 0.0, 0.0, 0.0))
TOKENS = dict(blank_bias=-60.0, duration_bias=(-30.0, 0.0, 0.0, 0.0, 0.0))

# The fixture of tests/test_gpu_parakeet_tdt.py and of the coverage test: weight sets (arguments, seed) and clips (set, T', frame
# seed).  The seeds are the lowest that tools/make_parakeet_tdt_golden.py --search accepts: the float64 paths have the coverage
# tests/test_pk_tdt_oracle.py asserts, and every step's top-two gaps are at least GAP_FACTOR times the float32 oracle's largest
# logit error on that path (the search asks for four times that).
GAP_FACTOR = 16.0
RAGGED_FRAMES = (0, 1, 2, 5, 31, 32, 33, 65)
FIXTURE_SETS = {"mix": (MIX, 27), "stall": (STALL, 1), "blanks": (BLANKS, 1), "tokens": (TOKENS, 1)}
FIXTURE_CLIPS = tuple(("mix", t, 100 + t) for t in RAGGED_FRAMES) + (("stall", 1, 201), ("stall", 3, 203), ("blanks", 7, 207), ("tokens", 7, 208))
GOLDEN_SEED = 27                 # tests/golden/parakeet_tdt_golden.npz: TINY_TDT, make_tdt_weights(TINY_TDT, GOLDEN_SEED, **MIX), frames(t, 256, t)
GOLDEN_FRAMES = (1, 5, 33)
CATALOG_FRAMES = (3, 40, 64)     # the catalog-width test: make_tdt_weights(CATALOG_TDT, CATALOG_SEED, **MIX), frames(t, 1024, 700 + t)
CATALOG_SEED = 2                 # the lowest that --search-catalog accepts, by the same rule


def make_tdt_weights(c: TdtConfig, seed: int, blank_bias: float = 4.0, duration_bias=(-4.0, 0.5, 0.0, 0.0, 0.0), head_gain: float = 2.0,
                     proj_gain: float = 1.5) -> dict:
    """seeded f32 weights by state-dict key: matrices / sqrt(fan-in) (the head times head_gain, the two projectors times proj_gain),
    the embedding of unit scale, biases about 0.1; the head's blank bias and duration biases are set to the arguments"""
    rng = np.random.default_rng(seed)
    out = {}
    for k, v in TdtModules(c).state_dict().items():
        shape = tuple(v.shape)
        if k.endswith("embedding.weight"):
            a = rng.standard_normal(shape)
        elif len(shape) == 1:
            a = 0.1 * rng.standard_normal(shape)
        else:
            a = rng.standard_normal(shape) / math.sqrt(shape[1])
            if k == "joint.head.weight":
                a *= head_gain
            elif k in ("encoder_projector.weight", "decoder.decoder_projector.weight"):
                a *= proj_gain
        out[k] = a.astype(np.float32)
    bias = out["joint.head.bias"]
    bias[c.blank] = blank_bias
    bias[c.vocab:] = np.asarray(duration_bias, np.float32)[:len(c.durations)]
    return out


class Tdt:
    """The decoder with `weights` (make_tdt_weights' form) in `dtype`, one clip [T'][H] at a time."""

    def __init__(self, c: TdtConfig, weights: dict, dtype=torch.float64):
        self.cfg, self.dtype = c, dtype
        self.net = TdtModules(c).to(dtype).eval()
        self.net.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)).to(dtype) for k, v in weights.items()}, strict=True)

    @torch.no_grad()
    def project(self, e) -> np.ndarray:
        """p = encoder_projector(e) as [T'][D] of the oracle's precision"""
        e = torch.from_numpy(np.ascontiguousarray(e, np.float32)).to(self.dtype)
        return self.net.encoder_projector(e).numpy().copy()

    def _predict(self, token, state):
        d = self.net.decoder
        out, state = d.lstm(d.embedding(torch.tensor([[int(token)]])), state)
        return d.decoder_projector(out)[0, 0], state

    def _start(self):
        c = self.cfg
        zero = torch.zeros(c.decoder_layers, 1, c.decoder_hidden, dtype=self.dtype)
        return self._predict(c.blank, (zero, zero.clone()))

    def _logits(self, p_t, g):
        return self.net.joint.head(torch.relu(p_t + g))

    @torch.no_grad()
    def decode(self, e, with_logits: bool = False):
        """the free-running loop -> steps int32 [n][3] (token, frame, duration); with_logits: also [n][V + n_d] of the oracle's precision"""
        c = self.cfg
        n_frames = int(np.asarray(e).shape[0])
        steps, rows = [], []
        if n_frames > 0:
            p = torch.from_numpy(self.project(e))
            g, state = self._start()
            t = 0
            for _ in range(max_steps(c, n_frames)):
                logits = self._logits(p[t], g)
                k = int(torch.argmax(logits[:c.vocab]))
                d = int(c.durations[int(torch.argmax(logits[c.vocab:]))])
                if k == c.blank and d == 0:
                    d = 1
                steps.append((k, t, d))
                rows.append(logits.numpy().copy())
                t += d
                if k != c.blank:
                    g, state = self._predict(k, state)
                if t >= n_frames:
                    break
        steps = np.asarray(steps, np.int32).reshape(-1, 3)
        if with_logits:
            return steps, np.asarray(rows).reshape(len(steps), c.width)
        return steps

    @torch.no_grad()
    def logits_along(self, e, steps) -> np.ndarray:
        """the logits [n][V + n_d] of the path `steps`, teacher-forced: each step's frame and token are taken from `steps`"""
        c = self.cfg
        steps = np.asarray(steps).reshape(-1, 3)
        rows = []
        if len(steps):
            p = torch.from_numpy(self.project(e))
            g, state = self._start()
            for k, t, _d in steps:
                rows.append(self._logits(p[int(t)], g).numpy().copy())
                if int(k) != c.blank:
                    g, state = self._predict(int(k), state)
        return np.asarray(rows).reshape(len(steps), c.width)


def top_two_gaps(logits: np.ndarray, vocab: int):
    """the smallest distance between the two largest token logits and between the two largest duration logits over the rows"""
    if not len(logits):
        return float("inf"), float("inf")
    tok = np.sort(logits[:, :vocab], axis=1)
    dur = np.sort(logits[:, vocab:], axis=1)
    return float((tok[:, -1] - tok[:, -2]).min()), float((dur[:, -1] - dur[:, -2]).min())


def raw_durations(logits: np.ndarray, c: TdtConfig) -> np.ndarray:
    """the predicted durations of the rows before the blank rule"""
    return np.asarray(c.durations)[np.argmax(logits[:, c.vocab:], axis=1)] if len(logits) else np.zeros(0, int)


def coverage(c: TdtConfig, paths) -> dict:
    """What the float64 paths [(T', steps, logits)] contain between them: the set of recorded durations, blanks whose predicted
    duration was 0, the longest run of non-blank tokens at one frame, clips that ended on the budget, the largest overshoot of T'."""
    got = dict(durations=set(), forced_blanks=0, longest_run=0, budget_ends=0, overshoot=0, blanks=0, tokens=0)
    for n_frames, steps, logits in paths:
        if not len(steps):
            continue
        raw = raw_durations(logits, c)
        blank = steps[:, 0] == c.blank
        got["durations"] |= set(int(d) for d in raw)
        got["forced_blanks"] += int((blank & (raw == 0)).sum())
        got["blanks"] += int(blank.sum())
        got["tokens"] += int((~blank).sum())
        run, at = 0, -1
        for (k, t, _d) in steps:
            run = run + 1 if (k != c.blank and t == at) else (1 if k != c.blank else 0)
            at = int(t)
            got["longest_run"] = max(got["longest_run"], run)
        end = int(steps[-1, 1] + steps[-1, 2])
        if end < n_frames:
            assert len(steps) == max_steps(c, n_frames)
            got["budget_ends"] += 1
        got["overshoot"] = max(got["overshoot"], end - n_frames)
    return got


def words(steps, pieces, n_frames: int, blank: int, seconds_per_frame: float = 0.08):
    """[(start_s, end_s, text)]: a piece that begins with U+2581 starts a word (and so does the first token), the marker is removed
    and pieces are concatenated; a word starts at its first token's frame and ends at its last token's min(frame + duration, T')"""
    out = []
    for k, t, d in np.asarray(steps).reshape(-1, 3):
        if int(k) == blank:
            continue
        piece = pieces[int(k)]
        start, end = int(t), min(int(t) + int(d), n_frames)
        fresh = piece.startswith(MARK)
        if fresh:
            piece = piece[len(MARK):]
        if fresh or not out:
            out.append([start, end, piece])
        else:
            out[-1][1] = end
            out[-1][2] += piece
    return [(np.float32(s * seconds_per_frame), np.float32(e * seconds_per_frame), text) for s, e, text in out]
