"""Record tests/golden/reduce_bits_parent.npz for tests/test_gpu_reduce_bits.py.

Run on an MI355X with the library the later work is compared against (the parent of the
change under test), from the repository root:

    python tests/golden/record_reduce_bits.py [output.npz]

Per case of the test the file holds its two seeds (data, positions) and the 64-bit
patterns of lp[8] and grad[8, D] as the library returned them; nothing else."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import test_gpu_reduce_bits as T   # noqa: E402


def main():
    out = {}
    for name in sorted(T.CASES):
        lp, g = T.evaluate(name)
        out[f"{name}/seeds"] = np.array(T.seeds(name), dtype=np.int64)
        out[f"{name}/lp_bits"] = lp.view(np.uint64).copy()
        out[f"{name}/grad_bits"] = g.view(np.uint64).copy()
        print(name, "D", g.shape[1], "lp", lp.tolist(), "finite grad:", bool(np.all(np.isfinite(g))))
    path = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
