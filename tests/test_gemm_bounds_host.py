"""tests/gemm_bounds.py checked on the CPU: a correct kernel, emulated as a torch f32 product of operands already rounded
to T that runs each epilogue in f32 and rounds once to T, stays inside the element-wise bound at every type and K; each
of the local faults the bound exists for makes the checker raise."""
import functools

import pytest
import torch

import gemm_bounds as gb
from conftest import rel_l2
from test_dispatch_map_gpu import NT_TOL

M, N = 1000, 256
PITCH, VALID = 101, 99                     # seams inside every tile height; rows 99, 100, 200, 201 ... are dead
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
KS = [64, 512, 4096]
EPILOGUES = ["bias", "relu", "glu", "mask", "glu_bwd", "glu_bwd_gate"]
FRAG = (976, 240)                          # a live 16 x 16 fragment of the last full slab of rows and columns


def _k_tile(dtype):
    return 32 if dtype == torch.float32 else 64       # the kernels' K step (csrc/gemm.hip: bk)


def _split(z):
    """[rows, 2 n] packed [16 a | 16 b] per 32 columns -> (a, b), each [rows, n]."""
    v = z.view(z.shape[0], -1, 2, 16)
    return v[:, :, 0].reshape(z.shape[0], -1), v[:, :, 1].reshape(z.shape[0], -1)


def _pack(a, b):
    out = torch.empty(a.shape[0], a.shape[1] // 16, 2, 16, dtype=a.dtype)
    out[:, :, 0], out[:, :, 1] = a.view(a.shape[0], -1, 16), b.view(b.shape[0], -1, 16)
    return out.view(a.shape[0], -1)


class Case:
    """Operands of one (dtype, K) and both sides of every epilogue."""

    def __init__(self, dtype, K):
        g = torch.Generator().manual_seed(K + 7 * DTYPES.index(dtype))
        rn = lambda *s: torch.randn(*s, generator=g)
        self.dtype, self.K = dtype, K
        self.A, self.W = rn(M, K).to(dtype), (rn(N, K) / K ** 0.5).to(dtype)
        self.bias = 0.1 * rn(N)
        self.res = rn(M, N).to(dtype)                 # residual (BIAS, GLU_BWD) / gating activation (MASK)
        self.res_glu = rn(M, N // 2).to(dtype)
        self.Z = rn(M, 2 * N).to(dtype)               # saved (a | b) of GLU_BWD, packed
        a, b = _split(self.Z.double())
        self.bg = b.to(dtype)                         # gate-only form: b and the saved output y
        self.y = (a * torch.sigmoid(b)).to(dtype)
        self.live = (torch.arange(M) % PITCH) < VALID
        self.acc32 = self.A.float() @ self.W.float().t()
        self.acc64 = self.A.double() @ self.W.double().t()

    def got(self, epi, acc=None, bias=None, db_sig_only=None):
        """What a correct kernel stores (dtype T).  acc / bias: a faulty accumulator / bias vector; db_sig_only: a
        (row, column) whose 16 x 16 fragment computes the db half with sig in place of sig (1 - sig)."""
        acc = self.acc32 if acc is None else acc
        bias = self.bias if bias is None else bias
        real = self.live[:, None]
        zero = torch.zeros((), dtype=torch.float32)
        if epi in ("bias", "relu", "mask"):
            v = acc + bias
            if epi == "relu":
                v = v.clamp_min(0)
            v = torch.where(real, v, zero)
            if epi == "bias":
                v = torch.where(real, v + self.res.float(), zero)
            if epi == "mask":
                v = torch.where(self.res.float() > 0, v, zero)
            return v.to(self.dtype)
        if epi == "glu":
            a, b = _split(acc + bias)
            o = torch.where(real, a * torch.sigmoid(b), zero)
            return torch.where(real, o + self.res_glu.float(), zero).to(self.dtype)
        d = torch.where(real, acc + self.res.float(), zero)
        if epi == "glu_bwd":
            a, b = _split(self.Z.float())
            sg = torch.sigmoid(b)
            da, db = d * sg, d * a * sg * (1 - sg)
            wrong = d * a * sg
        else:
            sg = torch.sigmoid(self.bg.float())
            da, db = d * sg, d * self.y.float() * (1 - sg)
            wrong = d * self.y.float()
        if db_sig_only is not None:
            r, c = db_sig_only
            db = db.clone()
            db[r:r + 16, c:c + 16] = wrong[r:r + 16, c:c + 16]
        return _pack(da, db).to(self.dtype)

    def want(self, epi):
        """(f64 result of the same rounded inputs, its element-wise bound, accumulator column of each output column)."""
        real = self.live[:, None]
        zero = torch.zeros((), dtype=torch.float64)
        bd = self.bias.double()
        cols = None
        if epi in ("bias", "relu", "mask"):
            v = self.acc64 + bd
            eps = gb.acc_error(gb.abs_sum(self.A, self.W, self.bias, self.res if epi == "bias" else None), self.K)
            if epi == "relu":
                v = v.clamp_min(0)
            if epi == "bias":
                v = v + self.res.double()
            if epi == "mask":
                gate = self.res.double() > 0
                v, eps = torch.where(gate, v, zero), torch.where(gate, eps, zero)
            want = torch.where(real, v, zero)
        elif epi == "glu":
            a, b = _split(self.acc64 + bd)
            ea, eb = _split(gb.acc_error(gb.abs_sum(self.A, self.W, self.bias), self.K))
            want = torch.where(real, a * torch.sigmoid(b) + self.res_glu.double(), zero)
            # the residual is added after the activation: an addend with L = 1
            eps = gb.glu_error(a, b, ea, eb) + gb.acc_error(self.res_glu.abs().double(), self.K)
            cols = gb.glu_acc_cols(N // 2)
        else:
            d = self.acc64 + self.res.double()
            ed = gb.acc_error(gb.abs_sum(self.A, self.W, None, self.res), self.K)
            if epi == "glu_bwd":
                a, b = _split(self.Z.double())
                sg = torch.sigmoid(b)
                da, db = d * sg, d * a * sg * (1 - sg)
                eda, edb = gb.glu_bwd_error(ed, b, a=a)
            else:
                b, y = self.bg.double(), self.y.double()
                sg = torch.sigmoid(b)
                da, db = d * sg, d * y * (1 - sg)
                eda, edb = gb.glu_bwd_error(ed, b, y=y)
            want, eps = torch.where(real, _pack(da, db), zero), _pack(eda, edb)
            cols = gb.glu_bwd_acc_cols(2 * N)
        return want, gb.element_bound(want, eps, self.dtype, live=self.live), cols

    def without_last_k_tile(self, frag=FRAG):
        """The f32 accumulator with one 16 x 16 fragment summed over all K tiles but the last."""
        r, c = frag
        k = self.K - _k_tile(self.dtype)
        acc = self.acc32.clone()
        acc[r:r + 16, c:c + 16] = self.A[r:r + 16, :k].float() @ self.W[c:c + 16, :k].float().t()
        return acc


@functools.lru_cache(maxsize=None)
def _case(dtype, K):
    return Case(dtype, K)


def _check(case, epi, got, tag):
    want, bound, cols = case.want(epi)
    return gb.check_elements(got, want, bound, tag, pitch=PITCH, acc_cols=cols)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_correct_kernel_stays_inside_the_bound(dtype, K):
    case = _case(dtype, K)
    for epi in EPILOGUES:
        worst = _check(case, epi, case.got(epi), f"{epi}[{dtype}:K{K}]")
        print(f"{epi}[{dtype}:K{K}] worst element / bound = {worst:.3f}")
        assert 0 < worst <= 1
    if K == 64 and dtype != torch.float32:
        # the bound is not slack: at a short K it is the half-ulp rounding itself
        assert _check(case, "bias", case.got("bias"), "tight") > 0.5


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_fragment_without_its_last_k_tile_raises(dtype, K):
    case = _case(dtype, K)
    for epi in EPILOGUES:
        got = case.got(epi, acc=case.without_last_k_tile())
        with pytest.raises(AssertionError, match=r"row 9[789]\d, column 2[2-5]\d.*256-tile \(3, 0\) fragment \(13, 1[45]\)"):
            _check(case, epi, got, f"dropped[{epi}:{dtype}:K{K}]")
    if K == 4096 and dtype == torch.bfloat16:
        # why the element-wise measure exists: the whole-tensor bound of the GPU tests accepts this output
        got = case.got("bias", acc=case.without_last_k_tile())
        want, bound, _ = case.want("bias")
        assert rel_l2(got, want) < NT_TOL[dtype]
        assert float(((got.double() - want).abs() / bound.clamp_min(1e-300)).max()) > 10


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_local_faults_of_the_plain_epilogue_raise(dtype, K):
    case = _case(dtype, K)
    good = case.got("bias")
    # one row replaced by its neighbour
    got = good.clone()
    got[500] = good[501]
    with pytest.raises(AssertionError, match=r"row 500, .*row % pitch = 96"):
        _check(case, "bias", got, "row")
    # one column's bias dropped
    c = int(case.bias.abs().argmax())
    bias = case.bias.clone()
    bias[c] = 0
    with pytest.raises(AssertionError, match=rf"column {c}, "):
        _check(case, "bias", case.got("bias", bias=bias), "bias")
    # one dead row left non-zero
    got = good.clone()
    got[PITCH + VALID] = good[PITCH + VALID - 1]
    with pytest.raises(AssertionError, match=rf"row {PITCH + VALID}, .*row % pitch = {VALID}.*bound 0.000e\+00"):
        _check(case, "bias", got, "dead row")
    # ... and one gated-off element of the ReLU gate
    gm = case.got("mask")
    off = (case.res[3].float() <= 0).nonzero()[0].item()
    gm[3, off] = good[3, off]
    with pytest.raises(AssertionError, match=rf"row 3, column {off}, "):
        _check(case, "mask", gm, "gated-off element")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_glu_backward_gate_half_with_the_wrong_derivative_raises(dtype, K):
    case = _case(dtype, K)
    for epi in ("glu_bwd", "glu_bwd_gate"):
        got = case.got(epi, db_sig_only=FRAG)
        with pytest.raises(AssertionError, match=r"256-tile \(3, 0\) fragment \(13, 15\)"):
            _check(case, epi, got, epi)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_one_element_four_roundings_off_raises(dtype):
    """K = 64, 16-bit T: the summation term is far below one rounding of T, so an element two units in the last place
    (four times the worst rounding error, half a unit) away from the correct kernel's is outside the bound.  (For f32
    outputs the worst-case summation term, 2 (K + 8) 2^-24 S, is itself a hundred roundings: no bound derived from worst
    cases can see this fault there.)"""
    case = _case(dtype, 64)
    got = case.got("bias")
    want, bound, _ = case.want("bias")
    flat = int(torch.where(case.live[:, None], want.abs(), torch.zeros(())).argmax())
    r, c = flat // N, flat % N
    bits = got.view(torch.int16)
    bits[r, c] += 2                                   # sign-magnitude: two units in the last place away from zero
    assert abs(float(got[r, c]) - float(want[r, c])) < 5 * gb.U[dtype] * abs(float(want[r, c]))
    with pytest.raises(AssertionError, match=rf"row {r}, column {c}, .*1 of {M * N} elements"):
        gb.check_elements(got, want, bound, "moved", pitch=PITCH)


def test_the_message_names_the_kernels_columns_and_chunked_rows():
    case = _case(torch.float16, 64)
    want, bound, cols = case.want("glu_bwd")
    got = case.got("glu_bwd")
    got[700, 2 * 64 + 16 + 3] += 1                    # db of accumulator column 64 + 3
    with pytest.raises(AssertionError, match=r"row 1700, column 67; .*64-tile \(26, 1\) fragment \(2, 0\) \(output column 147\)"):
        gb.check_elements(got, want, bound, "chunked", row0=1000, pitch=None, acc_cols=cols, chunk=256)
    got = case.got("bias")
    got[1, 1] = float("nan")
    want, bound, _ = case.want("bias")
    with pytest.raises(AssertionError, match="row 1, column 1; .*got nan"):
        gb.check_elements(got, want, bound, "nan")
