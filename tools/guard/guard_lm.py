"""The Transformer-LM kernels on the guard-page allocator (tools/guard/guard_alloc.cpp, set up as guard_pass.py does): the fused head with V = 1025 (tail column
tile, clamped rows of W and of h: R is not a multiple of the row tile) and the causal attention with sequence lengths that leave partial query / key tiles, in both
compute dtypes, on tensors of exactly the size the ABI documents.  A read or write past either end of a tensor faults.  Test infrastructure.
    GUARD_MODE=tail|head python tools/guard/guard_lm.py"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import torch


def main():
    so = os.path.join(HERE, "libguard_alloc.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(os.path.join(HERE, "guard_alloc.cpp")):
        subprocess.run(["hipcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "guard_alloc.cpp")], check=True)
    torch.cuda.memory.change_current_allocator(torch.cuda.memory.CUDAPluggableAllocator(so, "guard_malloc", "guard_free"))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from avec_amd import runtime as rt
    from avec_amd.lib import lib
    g = torch.Generator().manual_seed(0)
    for dt, tdt in ((0, torch.float32), (1, torch.bfloat16)):
        for R, V, D in ((77, 1025, 128), (64, 65, 64), (1, 1, 64)):
            h = torch.randn(R, D, generator=g).to(tdt).to(dev)
            W = torch.randn(V, D, generator=g).to(tdt).to(dev)
            bias, tgt, nll = torch.randn(V, generator=g).to(dev), torch.randint(-1, V, (R,), generator=g).to(dev), torch.empty(R, device=dev)
            lib.lm_head_nll(dt, h.data_ptr(), D, W.data_ptr(), D, bias.data_ptr(), tgt.data_ptr(), nll.data_ptr(), R, V, D, None, 0, rt.stream())
            torch.cuda.synchronize()
        for N, H, L in ((2, 2, 33), (1, 1, 130), (3, 1, 1)):
            qkv = torch.randn(N * L, 3 * H * 64, generator=g).to(tdt).to(dev)
            o = torch.empty(N * L, H * 64, dtype=tdt, device=dev)
            lens = torch.tensor(([L, 1, L // 2] * N)[:N], dtype=torch.int64, device=dev)
            lib.causal_attention(dt, qkv.data_ptr(), 3 * H * 64, lens.data_ptr(), o.data_ptr(), H * 64, N, H, L, 64, 0.125, rt.stream())
            torch.cuda.synchronize()
        ids = torch.randint(0, 65, (3, 17), generator=g).to(dev)
        E, P, out = torch.randn(65, 64, generator=g).to(dev), torch.randn(17, 64, generator=g).to(dev), torch.empty(3 * 17, 64, dtype=tdt, device=dev)
        lib.embed_pos(dt, ids.data_ptr(), E.data_ptr(), P.data_ptr(), out.data_ptr(), 0, 3, 17, 65, 64, rt.stream())
        torch.cuda.synchronize()
    import ctypes
    gl = ctypes.CDLL(so)
    gl.guard_stats.restype = ctypes.c_longlong
    print("GUARD LM OK mode=%s allocations=%d" % (os.environ.get("GUARD_MODE", "tail"), gl.guard_stats(0)), flush=True)


if __name__ == "__main__":
    main()
