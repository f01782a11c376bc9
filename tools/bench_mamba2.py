"""Mamba2 bottleneck (mamba_v2=True) on 1 x MI355X, one process: the chunked SSD scan at the E8-shaped config (B 16,
T 625, d_inner 2048 = 32 heads x 64, d_state 64) forward and backward in us per launch, the forward's share of HBM
bandwidth (algorithmic bytes: x, dt, B, C read once, y written once), and the Experiment_CleanU_Mamba2 forward at
B 32 x 10 s next to its Mamba1 sibling (442k).  GPU box only.  Prints one JSON line."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cleanumamba_amd import hip  # noqa: E402
from cleanumamba_amd.mamba_ssm.modules.mamba2 import _ssd_shape, mamba2_core  # noqa: E402
from cleanumamba_amd.network import CleanUMamba  # noqa: E402

HBM_GBS = 8000.0      # MI355X peak HBM3E bandwidth
dev = torch.device("cuda")


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def ckpt_net(name):
    with np.load(os.path.join(ROOT, "tests", "golden", f"ckpt_{name}.npz")) as f:
        cfg = json.loads(bytes(f["__network_config__"]).decode())
        sd = {k: torch.from_numpy(f[k].astype(np.float32)) for k in f.files if k != "__network_config__"}
    net = CleanUMamba(**cfg)
    net.load_state_dict(sd, strict=True)
    return net.to(dev).eval()


out = {}
B, T, H, P, N = 16, 625, 32, 64, 64
d = H * P
g = torch.Generator(device=dev).manual_seed(0)
lib = hip.lib()
for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
    xBC = torch.randn(B, T, d + 2 * N, generator=g, device=dev).to(dt)
    zx = torch.randn(B, T, 2 * d + 2 * N + H, generator=g, device=dev).to(dt)
    A_log, D = torch.log(torch.linspace(1, 16, H, device=dev)), torch.ones(H, device=dev)
    bias, w = torch.full((H,), -2.0, device=dev), torch.ones(d, device=dev)
    dtv = zx[..., -H:]
    y = torch.empty(B, T, d, dtype=dt, device=dev)
    st = torch.empty(lib.cum_ssd_states_elems(B, T, H, P, N), device=dev)
    s = _ssd_shape(xBC, dtv, xBC[..., d:], xBC[..., d + N:], y, H, P, N)
    fwd = lambda: hip.check(lib.cum_ssd_fwd(ctypes.byref(s), hip.ptr(xBC), hip.ptr(dtv), hip.ptr(bias), hip.ptr(A_log),
                                            hip.ptr(D), hip.ptr(xBC[..., d:]), hip.ptr(xBC[..., d + N:]), hip.ptr(y),
                                            hip.ptr(st), None, hip.stream_ptr()))
    ms = timeit(fwd)
    esz = xBC.element_size()
    nbytes = B * T * (esz * (2 * d + 2 * N + H))
    out[f"ssd_fwd_{name}_us"] = round(ms * 1e3, 1)
    out[f"ssd_fwd_{name}_hbm_fraction"] = round(nbytes / (ms * 1e-3) / 1e9 / HBM_GBS, 4)
    leaves = [t.clone().requires_grad_() for t in (xBC, zx, bias, A_log, D, w)]
    o = mamba2_core(*leaves, P, 1e-5)
    go = torch.randn_like(o)
    core_ms = timeit(lambda: torch.autograd.grad(mamba2_core(*leaves, P, 1e-5), leaves, go))
    out[f"ssd_core_fwd_bwd_{name}_us"] = round(core_ms * 1e3, 1)
    with torch.no_grad():
        out[f"ssd_core_fwd_{name}_us"] = round(timeit(lambda: mamba2_core(*leaves, P, 1e-5)) * 1e3, 1)
    out[f"ssd_bwd_{name}_us_approx"] = round((core_ms - out[f"ssd_core_fwd_{name}_us"] / 1e3) * 1e3, 1)

x = (0.1 * torch.randn(32, 1, 160000, generator=torch.Generator().manual_seed(3))).to(dev)
with torch.no_grad():
    for name in ("mamba2", "442k"):
        net = ckpt_net(name)
        out[f"forward_{name}_b32x10s_ms"] = round(timeit(lambda: net(x), iters=10), 2)
out["mamba2_over_mamba1"] = round(out["forward_mamba2_b32x10s_ms"] / out["forward_442k_b32x10s_ms"], 3)
print(json.dumps(out))
