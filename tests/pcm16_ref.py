"""The two int16 quantisers of util/denoise_eval.py stated in numpy on f32, and the values at which a quantiser goes
wrong (csrc/ragged.hip: cum_unframe_rows_ragged_pcm16, cum_pcm16_from_f32_ragged).

  mode 0   (y * 32767).clamp(-32768, 32767).to(torch.int16): the f32 product, clamped, truncated toward zero
  mode 1   (y * 32768).round().clamp(-32768, 32767):         the f32 product, rounded half to even, clamped
  NaN gives 0 in both modes; +-inf clamps.
"""
import numpy as np

F32 = np.float32


def quantise(v, mode):
    """int16 array of the f32 array ``v`` under ``mode`` (0 or 1)."""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == 0:
            w = np.trunc(np.clip(v * F32(32767), -32768, 32767))
        elif mode == 1:
            w = np.clip(np.rint(v * F32(32768)), -32768, 32767)
        else:
            raise ValueError("mode is 0 or 1")
    assert w.dtype == F32
    return np.where(np.isnan(w), F32(0), w).astype(np.int16)


def case_table(nan=True):
    """f32 values where a quantiser goes wrong: signs of zero, the ends of the range and one ulp past them, k / 32767 and
    k / 32768 with both f32 neighbours, the ties of mode 1, overshoot, infinities, NaN, the smallest subnormal."""
    one_up = F32(1) + F32(2.0 ** -23)
    v = [F32(0.0), F32(-0.0), F32(1), F32(-1), one_up, -one_up]
    for k in (1, 2, 3, 16383, 32766, 32767):
        for d in (32767, 32768):
            x = F32(k) / F32(d)
            for s in (F32(1), F32(-1)):
                v += [s * x, s * np.nextafter(x, F32(2)), s * np.nextafter(x, F32(0))]
    for t in (0.5, 1.5, 2.5):
        v += [F32(t / 32768), F32(-t / 32768)]
    v += [F32(-32768.5 / 32768), F32(2), F32(-2), F32(np.inf), F32(-np.inf), np.nextafter(F32(0), F32(1))]
    if nan:
        v.append(F32(np.nan))
    return np.array(v, F32)
