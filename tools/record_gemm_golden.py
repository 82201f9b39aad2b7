"""Record tests/golden/gemm_core_parent.npz: the bits gm_gemm_kernel (csrc/gemm.hip) gave BEFORE its K walk was reworked.

    python tools/record_gemm_golden.py [--lib PATH/libamc3d_hip.so] [--out tests/golden/gemm_core_parent.npz]

The fixture is made ONCE, from a library built from the parent commit of the K-walk rework, and never from the code under
test: tests/test_gpu_gemm_core.py compares the reworked kernel with it, so a fixture recorded from that kernel would prove
nothing.  The script therefore refuses to write when `git status` shows csrc/gemm.hip modified, and where the tree is no git
checkout (an exported copy) it insists on --lib, the parent-built library, whose SHA-256 goes into the fixture.

Per case (the list is CASES below, restated in the test, which checks that both agree) the operands are
numpy.random.default_rng(seed).uniform(-1, 1) as float32, seed = 1000 + the case's index; amc3d_gemm_probe runs the product
with the 128 x 128 tile; the fixture keeps a SHA-256 of the output bytes and the first 64 values, for the channel-major output
and, for the two conv products, the position-major rows (pm).
"""
import argparse
import ctypes
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEMM = "amcontrast3d_amd/csrc/gemm.hip"
FORWARD, BACKWARD_DATA, WGRAD = 0, 1, 2
KS = (64, 65, 79, 80, 81, 95, 96, 97, 136)          # channels on the K side of the conv products (N of the weight gradient)
PS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 200)   # positions: N of the conv products, K of the weight gradient
MS = (64, 72, 130)
BS = (1, 3)


def cases():
    """(product, b, M, P, K-side channels, strided) -- b = 3 takes the unaligned strided weight view (w + 3, ldw = cin + 3)"""
    out, i = [], 0
    for K in KS:
        for M in MS:
            for b in BS:
                for product in (FORWARD, BACKWARD_DATA):
                    out.append((product, b, M, PS[i % len(PS)], K, int(b == 3)))
                    i += 1
    for P in PS:
        for M in MS:
            for b in BS:
                out.append((WGRAD, b, M, P, KS[i % len(KS)], 0))
                i += 1
    # the split-K branch of the conv products beyond K = 136 (two ranges of 80 and 56): four ranges of 64, three of 80 / 80 / 40
    for product in (FORWARD, BACKWARD_DATA):
        out += [(product, 2, 256, 94, 256, 0), (product, 2, 256, 94, 256, 1), (product, 1, 130, 33, 200, 0)]
    return out


def operands(case, seed):
    """numpy float32 (weight block as (cout, cin) or dy, source) of a case, uniform in [-1, 1)"""
    import numpy as np
    product, b, M, P, K, _ = case
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(-1.0, 1.0, size=s).astype(np.float32)  # noqa: E731
    if product == WGRAD:
        return u(b, M, P), u(b, K, P)          # dy (b, cout, P), x (b, cin, P)
    cin, cout = (K, M) if product == FORWARD else (M, K)
    return u(cout, cin), u(b, K, P)            # w, x or dy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gemm_core_parent.npz"))
    a = ap.parse_args()
    git = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--", GEMM], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                         text=True)
    if git.returncode == 0 and git.stdout.strip():
        sys.exit(f"{GEMM} is modified: the fixture is recorded from the parent's kernel only; nothing written")
    if git.returncode != 0 and not a.lib:
        sys.exit("not a git checkout: name the parent-built library with --lib; nothing written")
    if a.lib:
        os.environ["AMC3D_LIB"] = os.path.abspath(a.lib)
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from amcontrast3d_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    sha, head, names = [], [], []
    cs = cases()
    for i, case in enumerate(cs):
        product, b, M, P, K, strided = case
        first, second = (torch.from_numpy(t).to(dev) for t in operands(case, 1000 + i))
        if product == WGRAD:
            cout, cin, ldw, nout = M, K, K, M * K
            wsb = int(lib.amc3d_pointwise_conv_workspace_bytes(b, cin, cout, P))
            src, other = first, second
        else:
            cin, cout = (K, M) if product == FORWARD else (M, K)
            ldw, nout = cin + 3 * strided, b * M * P
            if strided:
                base = torch.zeros(cout * ldw + 4, device=dev)
                torch.as_strided(base, (cout, cin), (ldw, 1), 3).copy_(first)
                first = base[3:]
            wsb = int(lib.amc3d_pointwise_conv_forward_workspace_bytes(b, cin, cout, P, 0) if product == FORWARD
                      else lib.amc3d_pointwise_conv_workspace_bytes(b, cin, cout, P))
            src, other = second, first
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
        for pm in ((0,) if product == WGRAD else (0, 1)):
            out = torch.zeros(nout, device=dev)
            _lib.check(lib.amc3d_gemm_probe(0, product, b, cin, cout, P, ldw, pm, p(src), p(other), p(out), p(ws) if wsb else None,
                                            wsb, stream()), "amc3d_gemm_probe")
            host = out.cpu().numpy()
            sha.append(hashlib.sha256(host.tobytes()).hexdigest())
            head.append(np.resize(host[:64], 64) if host.size >= 64 else np.concatenate([host, np.zeros(64 - host.size, np.float32)]))
            names.append(f"{i}:{pm}")
    with open(os.environ.get("AMC3D_LIB") or _lib._SO, "rb") as f:
        libsha = hashlib.sha256(f.read()).hexdigest()
    np.savez_compressed(a.out, cases=np.asarray(cs, dtype=np.int64), names=np.asarray(names), sha256=np.asarray(sha),
                        head=np.stack(head).astype(np.float32), library_sha256=np.asarray(libsha))
    print(f"{len(cs)} cases, {len(sha)} outputs -> {a.out}")


if __name__ == "__main__":
    main()
