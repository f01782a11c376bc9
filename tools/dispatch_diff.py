"""Host dispatch of two library builds side by side (no GPU needed): the tile / plan / workspace functions over a grid.

usage: python tools/dispatch_diff.py libA.so libB.so      prints the number of cases and every case that differs"""
import ctypes
import itertools
import sys

c_i32, c_i64 = ctypes.c_int32, ctypes.c_int64


class GemmDesc(ctypes.Structure):           # cum_gemm_desc (include/cleanumamba_hip.h)
    _fields_ = [("dtype", c_i32), ("epilogue", c_i32), ("M", c_i32), ("N", c_i32), ("K", c_i32),
                ("lda", c_i64), ("ldw", c_i64), ("ldc", c_i64), ("ldr", c_i64), ("ldz", c_i64),
                ("pitch", c_i32), ("valid", c_i32), ("n_store", c_i32), ("zero_head", c_i64), ("zero_tail", c_i64),
                ("gate_only", c_i32), ("ldy", c_i64), ("mask_bits", c_i32), ("allow_split_k", c_i32)]


def load(path):
    lib = ctypes.CDLL(path)
    lib.cum_gemm_nt_tile.argtypes = [ctypes.POINTER(GemmDesc)]
    for name in ("cum_gemm_tn_tile", "cum_gemm_tn_workspace_elems"):
        getattr(lib, name).argtypes = [c_i32, c_i64, c_i32, c_i32]
    for name in ("cum_scan_fwd_workspace_elems", "cum_scan_bwd_workspace_elems", "cum_scan_bwd_tp_workspace_elems"):
        getattr(lib, name).argtypes = [c_i32] * 4
    lib.cum_scan_fwd_keeps_y.argtypes = [c_i32] * 5
    for name in ("cum_gemm_tn_workspace_elems", "cum_scan_fwd_workspace_elems", "cum_scan_bwd_workspace_elems",
                 "cum_scan_bwd_tp_workspace_elems"):
        getattr(lib, name).restype = c_i64
    return lib


def cases(lib):
    MS = (1, 600, 10016, 40064, 320512, 1282048)
    NK = (16, 64, 128, 256, 384, 512, 768, 1024, 2048)
    for dt, M, N, K in itertools.product((0, 1, 2), MS, NK, NK):
        for sk in (0, 1, 2):
            d = GemmDesc(dtype=dt, M=M, N=N, K=K, allow_split_k=sk)
            yield ("nt_tile", dt, M, N, K, sk), lib.cum_gemm_nt_tile(ctypes.byref(d))
        yield ("tn_tile", dt, M, N, K), lib.cum_gemm_tn_tile(dt, M, N, K)
        yield ("tn_ws", dt, M, N, K), lib.cum_gemm_tn_workspace_elems(dt, M, N, K)
    for b, dim, n, length in itertools.product((1, 2, 3, 4, 16, 32, 128), (64, 128, 1024, 2048), (4, 8, 16, 17, 64),
                                               (16, 61, 96, 624, 2499, 10000)):
        yield ("scan_fwd_ws", b, dim, n, length), lib.cum_scan_fwd_workspace_elems(b, dim, n, length)
        yield ("scan_bwd_ws", b, dim, n, length), lib.cum_scan_bwd_workspace_elems(b, dim, n, length)
        yield ("scan_bwd_tp_ws", b, dim, n, length), lib.cum_scan_bwd_tp_workspace_elems(b, dim, n, length)
        for ws in (0, 1):
            yield ("scan_keeps_y", b, dim, n, length, ws), lib.cum_scan_fwd_keeps_y(b, dim, n, length, ws)


if __name__ == "__main__":
    a, b = load(sys.argv[1]), load(sys.argv[2])
    total = differ = 0
    for (key, va), (_, vb) in zip(cases(a), cases(b)):
        total += 1
        if va != vb:
            differ += 1
            print("DIFFERS", key, va, vb)
    print("%d cases, %d differ" % (total, differ))
    sys.exit(1 if differ else 0)
