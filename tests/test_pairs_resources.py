"""Register and LDS gate of the pairs plot's kernels (fitoct_amd/csrc/pairs_device.hip): the
-Rpass-analysis=kernel-resource-usage remarks fitoct_amd.build keeps beside the object show no
scratch, no spilled VGPR and at most 64 KiB of LDS for every kernel of it.
"""
from __future__ import annotations

import os
import subprocess

from fitoct_amd import build as B

KERNELS = ("digitise_kernel", "marginal_kernel", "panel_kernel", "mean_partial_kernel",
           "cov_partial_kernel", "slab_sum_kernel")


def _remarks():
    """The kept record, or a device-only recompile if it is missing or stale."""
    src = os.path.join(B.CSRC, "pairs_device.hip")
    path = os.path.join(B.OBJDIR, "pairs_device.resources.txt")
    if os.path.exists(path) and os.path.getmtime(path) >= B._newest_dep(src):
        return open(path).read()
    out = os.path.join("/tmp", f"fitoct_resources_pairs_{os.getpid()}.o")
    r = subprocess.run([B._hipcc(), *B._KERNEL, f"-I{B.INCLUDE}", f"-I{B.CSRC}",
                        "--cuda-device-only", "-c", src, "-o", out,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    os.remove(out)
    return r.stderr


def test_pairs_kernels_do_not_spill():
    rows = B.kernel_resources(_remarks())
    for kernel in KERNELS:
        assert len([k for k in rows if kernel in k]) == 1, (kernel, list(rows))
    # the shared kernels (staging, select) are the shared layer's object's alone
    assert len(rows) == len(KERNELS), list(rows)
    for kernel, r in rows.items():
        assert r.get("VGPRs Spill", -1) == 0 and r.get("ScratchSize", -1) == 0, (kernel, r)
        assert r.get("LDS Size", 1 << 30) <= 64 * 1024, (kernel, r)
    assert "pairs_device" in B.RECORDED and any(n == "pairs_device" for n, *_ in B.SOURCES)
