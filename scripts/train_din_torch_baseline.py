"""The DIN learning test's threshold (tests/test_train_din.py::test_it_learns): torch.optim.Adam(eps=1e-7) on the CPU, on the graph and
the exact arrays of tests/train_din_cases.py (planted(), DIN at the reference widths, batch 256, 5 epochs, lr 0.01), over five seeds.
Prints per seed the epoch losses and the held-out rank AUC before and after, then lowest - (max - min): the threshold the test uses.

    python scripts/train_din_torch_baseline.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.nn.functional as Fn

    from sparrowrecsys_amd import trainer_din as TD
    from sparrowrecsys_amd.metrics import exact_roc_auc
    from tests import train_din_cases as TDC
    (ids, dense, y), (tids, tdense, ty) = TDC.planted()
    ids_t, dn, y_t = torch.from_numpy(ids.astype(np.int64)), torch.from_numpy(dense), torch.from_numpy(y)
    tids_t, tdn = torch.from_numpy(tids.astype(np.int64)), torch.from_numpy(tdense)
    aucs = []
    for seed in range(5):
        model = TDC.planted_model(seed)
        fam = TD.family_of(model)
        p = {k: torch.tensor(np.array(model.weights[k]), requires_grad=True) for k in TD.param_names(fam)}
        opt = torch.optim.Adam(list(p.values()), lr=0.01, eps=1e-7)
        with torch.no_grad():
            before = exact_roc_auc(ty, torch.sigmoid(TDC.torch_logit(fam, p, tids_t, tdn, torch.float32)).numpy())
        losses = []
        for _ in range(5):
            tot = 0.0
            for b0 in range(0, len(y), 256):
                opt.zero_grad()
                loss = Fn.binary_cross_entropy_with_logits(TDC.torch_logit(fam, p, ids_t[b0:b0 + 256], dn[b0:b0 + 256], torch.float32), y_t[b0:b0 + 256])
                loss.backward()
                opt.step()
                tot += float(loss.detach()) * len(y_t[b0:b0 + 256])
            losses.append(tot / len(y))
        with torch.no_grad():
            after = exact_roc_auc(ty, torch.sigmoid(TDC.torch_logit(fam, p, tids_t, tdn, torch.float32)).numpy())
        aucs.append(after)
        print("seed %d: losses %s falling %s, held-out AUC %.4f -> %.4f" % (seed, " ".join("%.4f" % l for l in losses),
                                                                             all(b < a for a, b in zip(losses, losses[1:])), before, after))
    print("lowest %.4f, spread %.4f, threshold = lowest - spread = %.4f" % (min(aucs), max(aucs) - min(aucs), min(aucs) - (max(aucs) - min(aucs))))


if __name__ == "__main__":
    main()
