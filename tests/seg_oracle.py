"""Oracle of the segmentation network (crispy_diar_seg_*, include/crispy_hip.h): pyannote segmentation-3.0 ("PyanNet")
restated as torch.nn modules on the CPU, constructible in float32 and in float64, and seeded weights for it.

  wav_norm1d InstanceNorm1d(1, affine) -> conv1d.0: 80 filters x 251 taps, stride 10, no bias, abs, MaxPool1d(3), InstanceNorm1d(80,
  affine), leaky_relu -> conv1d.1: Conv1d(80, 60, 5), pool, norm, leaky_relu -> conv1d.2: Conv1d(60, 60, 5), pool, norm,
  leaky_relu -> LSTM(60, 128, 4 layers, bidirectional) -> Linear(256, 128), leaky_relu, Linear(128, 128), leaky_relu ->
  Linear(128, 7), log_softmax.

The weights come from numpy.random.default_rng(seed), never from torch's generator: name -> float32 array under pyannote's
state-dict keys, `sincnet.conv1d.0.filters` being the evaluated [80, 1, 251] filter bank.  The same dict goes into the oracle
and into Diarizer.load_segmentation."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.fbank_oracle import segmentation_windows      # noqa: F401  (pyannote_get_segments_fixed:103-128, restated there)

WIN, N_CLASSES, HIDDEN, LAYERS = 160000, 7, 128, 4
CLASSIFIER_SCALE = 4096.0      # the classifier's weights are drawn from U(+-1/sqrt(128)) times this, so that the decisions move with the input


def n_frames(n: int) -> int:
    """rows the network gives for n samples (0 where a layer would be left without input)"""
    if n < 251:
        return 0
    c2 = (((n - 251) // 10 + 1) // 3 - 4) // 3 - 4
    return c2 // 3 if c2 > 0 else 0


def pool_remainders(n: int):
    """(c0 % 3, c1 % 3, c2 % 3): what each of the three MaxPool1d(3) floors drops"""
    c0 = (n - 251) // 10 + 1
    c1 = c0 // 3 - 4
    c2 = c1 // 3 - 4
    return c0 % 3, c1 % 3, c2 % 3


def make_weights(seed: int, classifier_seed=None) -> dict:
    """Every tensor from numpy.random.default_rng(seed); with `classifier_seed` the classifier's two from a generator of their own
    (the end-to-end fixture picks it so that the float64 oracle's decisions are spread and clear)."""
    rng = np.random.default_rng(seed)

    def uni(shape, fan):
        b = 1.0 / np.sqrt(fan)
        return rng.uniform(-b, b, shape).astype(np.float32)

    w = {"sincnet.wav_norm1d.weight": rng.uniform(0.8, 1.2, 1).astype(np.float32),
         "sincnet.wav_norm1d.bias": rng.uniform(-0.1, 0.1, 1).astype(np.float32)}
    # random band-limited rows: a windowed difference of two sinc low-passes, like the bank ParamSincFB evaluates
    t = np.arange(-125, 126, dtype=np.float64) / 16000.0
    win = np.hamming(251)
    lo = np.sort(rng.uniform(30.0, 6000.0, 80))
    band = rng.uniform(50.0, 1500.0, 80)
    rows = []
    for a, b in zip(lo, band):
        hi = min(a + b, 7900.0)
        r = (2 * hi * np.sinc(2 * hi * t) - 2 * a * np.sinc(2 * a * t)) * win
        rows.append(r / np.abs(r).max() * rng.uniform(0.5, 1.0))
    w["sincnet.conv1d.0.filters"] = np.asarray(rows, np.float32).reshape(80, 1, 251)
    w["sincnet.conv1d.1.weight"] = uni((60, 80, 5), 80 * 5)
    w["sincnet.conv1d.1.bias"] = uni(60, 80 * 5)
    w["sincnet.conv1d.2.weight"] = uni((60, 60, 5), 60 * 5)
    w["sincnet.conv1d.2.bias"] = uni(60, 60 * 5)
    for i, c in enumerate((80, 60, 60)):
        w[f"sincnet.norm1d.{i}.weight"] = rng.uniform(0.8, 1.2, c).astype(np.float32)
        w[f"sincnet.norm1d.{i}.bias"] = rng.uniform(-0.2, 0.2, c).astype(np.float32)
    for layer in range(LAYERS):
        n_in = 60 if layer == 0 else 2 * HIDDEN
        for tail in (f"_l{layer}", f"_l{layer}_reverse"):
            w["lstm.weight_ih" + tail] = uni((4 * HIDDEN, n_in), HIDDEN)
            w["lstm.weight_hh" + tail] = uni((4 * HIDDEN, HIDDEN), HIDDEN)
            w["lstm.bias_ih" + tail] = uni(4 * HIDDEN, HIDDEN)
            w["lstm.bias_hh" + tail] = uni(4 * HIDDEN, HIDDEN)
    w["linear.0.weight"] = uni((128, 256), 256)
    w["linear.0.bias"] = uni(128, 256)
    w["linear.1.weight"] = uni((128, 128), 128)
    w["linear.1.bias"] = uni(128, 128)
    if classifier_seed is not None:
        rng = np.random.default_rng(classifier_seed)
    w["classifier.weight"] = uni((N_CLASSES, 128), 128) * np.float32(CLASSIFIER_SCALE)
    w["classifier.bias"] = uni(N_CLASSES, 128)
    return w


class InstanceNorm(torch.nn.Module):
    """InstanceNorm1d(c, affine=True) at inference without running statistics: the mean and the biased variance over time, eps
    1e-5.  Written out because torch.nn.InstanceNorm1d refuses a single time step (a window of 991 samples has one frame)."""

    def __init__(self, c):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(c))
        self.bias = torch.nn.Parameter(torch.zeros(c))

    def forward(self, x):
        mean = x.mean(-1, keepdim=True)
        var = x.var(-1, unbiased=False, keepdim=True)
        return (x - mean) / torch.sqrt(var + 1e-5) * self.weight[:, None] + self.bias[:, None]


class PyanNet(torch.nn.Module):
    def __init__(self, weights: dict, dtype=torch.float64):
        super().__init__()
        self.wav_norm = InstanceNorm(1)
        self.norms = torch.nn.ModuleList([InstanceNorm(c) for c in (80, 60, 60)])
        self.conv1 = torch.nn.Conv1d(80, 60, 5)
        self.conv2 = torch.nn.Conv1d(60, 60, 5)
        self.lstm = torch.nn.LSTM(60, HIDDEN, num_layers=LAYERS, bidirectional=True, batch_first=True)
        self.linear = torch.nn.ModuleList([torch.nn.Linear(256, 128), torch.nn.Linear(128, 128)])
        self.classifier = torch.nn.Linear(128, N_CLASSES)
        self.to(dtype)
        t = {k: torch.from_numpy(np.asarray(v, np.float32)).to(dtype) for k, v in weights.items()}
        self.filters = t["sincnet.conv1d.0.filters"].reshape(80, 1, 251)
        with torch.no_grad():
            self.wav_norm.weight.copy_(t["sincnet.wav_norm1d.weight"])
            self.wav_norm.bias.copy_(t["sincnet.wav_norm1d.bias"])
            for i, nm in enumerate(self.norms):
                nm.weight.copy_(t[f"sincnet.norm1d.{i}.weight"])
                nm.bias.copy_(t[f"sincnet.norm1d.{i}.bias"])
            for i, cv in ((1, self.conv1), (2, self.conv2)):
                cv.weight.copy_(t[f"sincnet.conv1d.{i}.weight"])
                cv.bias.copy_(t[f"sincnet.conv1d.{i}.bias"])
            for name, p in self.lstm.named_parameters():
                p.copy_(t["lstm." + name])
            for i, ln in enumerate(self.linear):
                ln.weight.copy_(t[f"linear.{i}.weight"])
                ln.bias.copy_(t[f"linear.{i}.bias"])
            self.classifier.weight.copy_(t["classifier.weight"])
            self.classifier.bias.copy_(t["classifier.bias"])
        self.dtype = dtype
        self.eval()

    @torch.no_grad()
    def forward(self, windows):
        """windows [n_win, len] -> (scores [n_win, frames, 7], sincnet [n_win, frames, 60], lstm [n_win, frames, 256]) as numpy"""
        x = torch.as_tensor(np.asarray(windows, np.float32)).to(self.dtype).unsqueeze(1)
        x = self.wav_norm(x)
        x = torch.abs(F.conv1d(x, self.filters, stride=10))
        x = F.leaky_relu(self.norms[0](F.max_pool1d(x, 3, 3)))
        x = F.leaky_relu(self.norms[1](F.max_pool1d(self.conv1(x), 3, 3)))
        x = F.leaky_relu(self.norms[2](F.max_pool1d(self.conv2(x), 3, 3)))
        sinc = x.transpose(1, 2)
        lstm, _ = self.lstm(sinc)
        y = lstm
        for ln in self.linear:
            y = F.leaky_relu(ln(y))
        scores = F.log_softmax(self.classifier(y), dim=-1)
        return scores.numpy(), sinc.contiguous().numpy(), lstm.numpy()

    def scores(self, windows):
        return self.forward(windows)[0]
