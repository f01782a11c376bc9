"""Element-wise error bound of ONE cum_gemm_nt call: every output element against its own budget, so that a local error
(one fragment of an edge tile, the last wave slab of a ragged M, a column group beyond n_store, the row next to a
pitch / valid seam, a stale LDS stage in one tile) cannot hide in a whole-tensor average.  Plain torch; runs on whatever
device its arguments live on.

Derivation.  The kernels accumulate exact products of operands that are already rounded to the element type T into an
f32 accumulator, run the epilogue in f32 and round ONCE to T.  For one accumulator element

    acc = sum_k a_k w_k (+ bias) (+ res)

let S = sum_k |a_k||w_k| + |bias| + |res| (abs_sum(): an f32 product of the absolute values inflated by 1 %, which pays
for its own summation error, K 2^-24 < 1 % up to K = 160 000; S only has to be an upper bound).

  * Summation.  Any order of K + O(1) f32 additions of exact products errs by at most (K + 8) 2^-24 S to first order
    (each partial sum is bounded by S and every addition rounds it once; the 8 pays for the bias, the residual and the
    hand-over of partial sums between waves or K splits).  An MFMA accumulate need not round like a chain of IEEE
    additions (wider internal sums, one rounding per 4..32 products), which the factor 2 covers:

        eps_acc = 2 (K + 8) 2^-24 S                                                                  (acc_error())

  * Epilogue.  With f the epilogue as a function of the accumulator(s), an accumulator error of eps_acc moves the result
    by eps_acc L, L = |df / dacc| evaluated in f64 on the inputs the reference uses:
        BIAS, RELU, MASK and their ungated / pre-activation aux copies: L = 1 (ReLU and the gate are 1-Lipschitz; a gated-off
            element has L = 0: it is an exact zero),
        GLU  a sig(b): eps_a sig(b) + |a| sig(b) (1 - sig(b)) eps_b, each accumulator with its own S            (glu_error()),
        GLU_BWD: sig(b) for the da half; |a| sig (1 - sig) for the db half in the packed form, |y| (1 - sig) in the
            gate-only form; the gate, a and y are 16-bit inputs and therefore exact                         (glu_bwd_error()).
    The epilogue's own f32 multiplications (at most four roundings, 2^-22 relative) and the hardware exp / reciprocal
    inside sigmoid (1 ulp each, plus the rounding of the exponent's argument) are paid by 2^-20 |want|.  The
    subtraction 1 - sig(b) turns an absolute sigmoid error of c 2^-24 (c about 2: the rounding of 1 + e^-b and of the
    reciprocal) into a relative c 2^-24 / (1 - sig) of the db half.  For 16-bit T that is below u(T) for every gate
    b < 8.  For f32 it has no term of its own: it is inside eps_acc L (>= 2 (K + 8) 2^-24 |want|, as S >= |d|) while
    c / (1 - sig) < 2 (K + 8) S / |d|, which a gate of unit variance (b < 6: 1 / (1 - sig) < 404) and a gradient that is
    a sum of K >= 64 products of mixed sign (S / |d| of the order of sqrt(K)) satisfy.  An f32 db element that ever exceeds its bound at a
    large positive gate calls for this derivation to become a term, not for a measured widening.

  * Output rounding.  Round-to-nearest into T errs by at most u(T) |x|: bf16 2^-8, f16 2^-11, f32 2^-24; below the
    normal range of f16 the spacing is 2^-24 whatever |x| (floor(f16) = 2^-24; bf16 and f32 keep f32's exponent range:
    floor 0).

        bound_e = u(T) |want_e| + eps_acc L_e + 2^-20 |want_e| + floor(T)                              (element_bound())

Rows outside a clip (m % pitch >= valid) are stored as exact zeros: their bound is 0.

No term comes from an error measured on a GEMM.  A term may be widened only by a derivation from the documented accuracy
of the instructions involved, written down here.
"""
import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
FLOOR = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -24, torch.float32: 0.0}
TRANSCENDENTAL = 2.0 ** -20


def abs_sum(A, W, bias=None, res=None):
    """S [M, N] (f64) >= sum_k |A[m, k]| |W[n, k]| + |bias[n]| + |res[m, n]|."""
    S = (A.abs().float() @ W.abs().float().t()).double() * 1.01
    if bias is not None:
        S = S + bias.abs().double()
    if res is not None:
        S = S + res.abs().double()
    return S


def acc_error(S, K):
    """eps_acc: worst-case error of the f32 accumulator whose absolute sum is S."""
    return 2.0 * (K + 8) * 2.0 ** -24 * S


def glu_error(a, b, eps_a, eps_b):
    """eps_acc L of a * sig(b); a, b: the exact (f64) accumulators."""
    sg = torch.sigmoid(b)
    return eps_a * sg + a.abs() * sg * (1 - sg) * eps_b


def glu_bwd_error(eps_d, b, a=None, y=None):
    """(eps L of the da half, of the db half) of the GLU backward of a gradient d with accumulator error eps_d;
    packed form: pass the saved pre-activation a, gate-only form: the saved output y."""
    sg = torch.sigmoid(b)
    return eps_d * sg, eps_d * (a.abs() * sg * (1 - sg) if y is None else y.abs() * (1 - sg))


def element_bound(want, eps_l, dtype, live=None):
    """bound_e; eps_l = eps_acc L_e; live [rows] bool: rows that are not stored as zeros."""
    w = want.double().abs()
    bound = (U[dtype] + TRANSCENDENTAL) * w + eps_l + FLOOR[dtype]
    if live is not None:
        bound = torch.where(live.reshape(-1, 1), bound, torch.zeros_like(bound))
    return bound


def _where(row, col, pitch):
    s = f"row {row}, column {col}"
    if pitch is not None:
        s += f", row % pitch = {row % pitch}"
    for t in (256, 128, 64):
        s += f"; {t}-tile ({row // t}, {col // t}) fragment ({row % t // 16}, {col % t // 16})"
    return s


def check_elements(got, want, bound, tag, row0=0, pitch=None, acc_cols=None, chunk=32768):
    """Assert |got - want| <= bound for every element ([rows, cols]; a bound of 0 demands equality); -> the worst ratio.
    row0: the row of the whole output that row 0 of these tensors is (callers that walk row chunks); pitch: the clip
    pitch, for the message; acc_cols [cols]: accumulator column of each output column where the epilogue packs or pairs
    columns (GLU, GLU_BWD), so that the tile coordinates in the message are the kernel's."""
    assert got.shape == want.shape == bound.shape and got.dim() == 2, (tag, got.shape, want.shape, bound.shape)
    worst = 0.0
    for lo in range(0, got.shape[0], chunk):
        g, w, b = got[lo:lo + chunk].double(), want[lo:lo + chunk].double(), bound[lo:lo + chunk].double()
        diff = (g - w).abs()
        ratio = torch.nan_to_num(diff / b.clamp_min(1e-300), nan=float("inf"), posinf=float("inf"))
        top = float(ratio.max()) if ratio.numel() else 0.0
        if not top <= 1.0:
            i = int(ratio.argmax())
            r, c = i // ratio.shape[1], i % ratio.shape[1]
            row, col = row0 + lo + r, c if acc_cols is None else int(acc_cols[c])
            raise AssertionError(
                f"{tag}: element over its bound by {top:.3g}x at {_where(row, col, pitch)}"
                f"{'' if acc_cols is None else f' (output column {c})'}: got {float(g[r, c])!r}, want {float(w[r, c])!r}, "
                f"bound {float(b[r, c]):.3e}; {int((ratio > 1).sum())} of {ratio.numel()} elements of rows "
                f"{row0 + lo}..{row0 + lo + ratio.shape[0] - 1} exceed theirs")
        worst = max(worst, top)
    return worst


def glu_acc_cols(n_out, device=None):
    """Output column oc of the GLU epilogue -> the accumulator column of its a half (weights are packed [16 a | 16 b])."""
    oc = torch.arange(n_out, device=device)
    return 32 * (oc // 16) + oc % 16


def glu_bwd_acc_cols(n_out, device=None):
    """Output column zc of the GLU_BWD epilogue (Z's layout: [16 da | 16 db] per 16 accumulator columns) -> that column."""
    zc = torch.arange(n_out, device=device)
    return 16 * (zc // 32) + zc % 16
