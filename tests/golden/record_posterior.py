"""Record the fixtures that pin the posterior tables across a restructuring of their code,
with the library the later work is compared against (the parent of the change under test),
from the repository root:

    python tests/golden/record_posterior.py refusals   # no GPU: posterior_refusals.json
    python tests/golden/record_posterior.py tables     # on an MI355X: the three .npy tables

``refusals``: status and fitoct_last_error() text of every case of
tests/test_posterior_refusals.py.  ``tables``: the device tables that
test_gpu_monitor.py::test_monitor_table_is_unchanged (monitor cases a and i) and
test_gpu_curves.py::test_curves_table_is_unchanged (curves case b, one pass) compare bit for
bit, as the library returned them; nothing else."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def refusals():
    import test_posterior_refusals as T
    with open(T.FIXTURE, "w") as f:
        json.dump(T.record(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", T.FIXTURE)


def tables():
    import torch

    import curves_cases as CC
    import monitor_cases as MC
    from fitoct_amd.api import curves_device, monitor_device

    def save(name, table):
        path = os.path.join(HERE, name)
        np.save(path, table)
        print("wrote", path, table.shape, os.path.getsize(path), "bytes,",
              int(np.isnan(table).sum()), "NaN")

    for k in ("a", "i"):
        case = MC.CASES[k]()
        t = torch.from_numpy(case.raw).to("cuda")
        _, C_, I, _ = case.raw.shape
        save(f"monitor_case_{k}.npy",
             monitor_device(t.data_ptr(), case.probs_list, C_, I, case.first_iter))
    case = CC.CASES["b"]()
    t = torch.from_numpy(case.raw).to("cuda")
    _, C_, I, _ = case.raw.shape
    save("curves_case_b.npy", curves_device(t.data_ptr(), case.probs_list, C_, I,
                                            case.first_iter, case.probs, case.what))


if __name__ == "__main__":
    {"refusals": refusals, "tables": tables}[sys.argv[1]]()
