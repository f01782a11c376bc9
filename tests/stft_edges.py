"""Inputs and the guard condition of the STFT-loss edge tests (tests/test_stft_edges_host.py, tests/test_stft_edges_gpu.py).
Plain torch on the CPU.

The loss takes sqrt(clamp(re^2 + im^2, 1e-7)) of every bin, and the gradient wrt the spectrum is cut to zero below the
clamp: it is DISCONTINUOUS there.  A bin whose power lies within rounding of 1e-7 can be live in f32 and dead in f64 (or
the other way round), and one such bin carries a 1 / |X| ~ 3000x typical contribution to the log-magnitude gradient.  No
tolerance covers that, so gradient tests do not depend on such a bin: before they touch the GPU they assert, in f64, that
no bin of either signal at any resolution they use has a power in (0.9e-7, 1.1e-7) -- guard_count(...) == 0.

Why +-10 %: for a full-scale frame of these inputs (0.05 * randn under a Hann window of up to 2048 points) the f32
spectrum errs by about 6e-8 * 5 * sqrt(sum (w x)^2) ~ 1.3e-7 in amplitude; the clamp amplitude is 3.16e-4, so the power
of a bin at the clamp moves by about 8e-4 relative: +-10 % leaves ~100x margin.  The seeds are picked on the CPU; should a
torch update change the random stream, the guard assert fails loudly instead of the comparison turning flaky.  Values
need no guard: the loss is continuous across the clamp.
"""
import torch

# the reference's three resolutions, (n_fft, hop, win_length), in the order the existing tests configure them
STANDARD = ((512, 50, 240), (1024, 120, 600), (2048, 240, 1200))
CLAMP = 1e-7
B, L, SPAN = 2, 6000, (1500, 4200)        # the silence cases


def bin_powers(x64, n_fft, hop, win):
    """re^2 + im^2 of torch.stft in float64, (B, bins, frames), under the f32-valued Hann window cast to f64 exactly as
    oracle/cleanumamba_ref.py::mrstft_loss_ref builds it."""
    assert x64.dtype == torch.float64
    w = torch.hann_window(win, dtype=torch.float32).to(torch.float64)
    s = torch.stft(x64, n_fft, hop, win, w, return_complex=True)
    return s.real ** 2 + s.imag ** 2


def guard_count(x64, resolutions, lo=0.9e-7, hi=1.1e-7):
    """Number of bins, over all resolutions, whose power lies strictly between lo and hi."""
    n = 0
    for n_fft, hop, win in resolutions:
        p = bin_powers(x64, n_fft, hop, win)
        n += int(((p > lo) & (p < hi)).sum())
    return n


def max_power(x64, resolutions):
    return max(float(bin_powers(x64, *r).max()) for r in resolutions)


def pair(B, L, seed):
    """clean = 0.05 randn, den = clean + 0.05 randn, drawn in f32 so that the GPU and the f64 oracle see the same values."""
    g = torch.Generator().manual_seed(seed)
    clean = 0.05 * torch.randn(B, L, generator=g)
    return clean, clean + 0.05 * torch.randn(B, L, generator=g)


def faint(B, L, seed, scale=1e-6):
    return scale * torch.randn(B, L, generator=torch.Generator().manual_seed(seed))


def silenced(x, lo, hi, rows=None):
    """A copy of x with samples [lo, hi) of every row (or of `rows`) set to exact 0.0 -- digital silence."""
    x = x.clone()
    if rows is None:
        x[:, lo:hi] = 0.0
    else:
        x[rows, lo:hi] = 0.0
    return x


# name -> builder(seed) -> (clean, den) of the silence cases (B, L and SPAN above)
def _span(which):
    def build(seed):
        clean, den = pair(B, L, seed)
        return (silenced(clean, *SPAN) if "clean" in which else clean,
                silenced(den, *SPAN) if "den" in which else den)
    return build


SILENCE = {
    "den_span": _span(("den",)),
    "clean_span": _span(("clean",)),
    "both_span": _span(("clean", "den")),
    "den_zero": lambda seed: (pair(B, L, seed)[0], torch.zeros(B, L)),
    "den_faint": lambda seed: (pair(B, L, seed)[0], faint(B, L, seed + 100)),
    "clean_zero": lambda seed: (torch.zeros(B, L), pair(B, L, seed)[1]),
}
SILENCE_SEED = 3          # guard count 0 for clean, den and both with the span silenced (also at 4, 5, 6; not 0, 1, 2, 7)

# Single-resolution geometries, name -> (n_fft, hop, win, B, L, seed).  Each seed is the first from 3 up whose clean and
# den both have guard count 0 at that resolution (seed 3 of hop_gt_win has one bin in the band).
GEOMETRY = {
    "odd_hop_odd_win": (1024, 125, 599, 2, 3001, 3),       # fused; element-wise loads, window ends inside a pair
    "odd_offset": (1024, 125, 598, 2, 3001, 3),            # fused; off = 213: the pair that straddles the window start
    "odd_win_off0": (512, 77, 511, 2, 3001, 3),            # fused; off = 0 by floor
    "win_eq_nfft": (2048, 240, 2048, 2, 3001, 3),          # fused; window = n_fft
    "hop_gt_win": (512, 300, 240, 2, 3001, 4),             # fused; 20 % of the samples lie under no frame
    "rocfft128": (256, 64, 256, 2, 3001, 3),               # not fused: rocFFT of 128 points
    "short512": (512, 50, 240, 2, 257, 3),                 # the shortest legal clips, L = n_fft / 2 + 1: every frame
    "short1024": (1024, 120, 600, 2, 513, 3),              # reflects at both ends
}


def geometry(name):
    """((n_fft, hop, win),), clean, den of one GEOMETRY entry."""
    n_fft, hop, win, b, length, seed = GEOMETRY[name]
    return (((n_fft, hop, win),),) + pair(b, length, seed)


HALF_EQUAL_FROM = 2400


def half_equal(seed=3):
    """den == clean from sample 2400 on: over every frame of the `high` band of the three standard resolutions at L = 6000
    (the earliest sample such a frame sees is 13 * 240 - 600 = 2520), different before it."""
    clean, den = pair(B, L, seed)
    den[:, HALF_EQUAL_FROM:] = clean[:, HALF_EQUAL_FROM:]
    return clean, den


def loss_fn_batch(seed=3):
    """(3, 1, 6000) clean and den for loss_fn: clip 0's clean all zero, clip 1's den silent in its second half."""
    clean, den = pair(3, L, seed)
    clean[0] = 0.0
    den[1, L // 2:] = 0.0
    return clean.unsqueeze(1), den.unsqueeze(1)


def ref_kwargs(resolutions, band):
    return dict(fft_sizes=tuple(r[0] for r in resolutions), hop_sizes=tuple(r[1] for r in resolutions),
                win_lengths=tuple(r[2] for r in resolutions), band=band)
