"""The pair-dot DeepFM learning test's threshold (tests/test_train_pair.py::test_it_learns_what_only_the_dots_carry): torch.optim.Adam(eps=1e-7)
on the CPU, on the graph and the exact arrays of tests/train_pair_cases.py (learning(): label = (movieId + userId) mod 2, constant numerics,
deep_emb on a field the label ignores, batch 64, 40 epochs, lr 0.02), over five initialisation seeds.  Prints per seed the final training
AUC, then worst - (best - worst): the threshold the test uses.

    python scripts/train_pair_torch_baseline.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests import train_pair_cases as TPC
    aucs = []
    for seed in range(5):
        fam, w, ids, dense, y = TPC.learning(seed)
        aucs.append(TPC.torch_adam_fit(fam, w, ids, dense, y, 64, 40, 0.02))
    print("final training AUCs %s; worst %.4f, spread %.4f, threshold = worst - spread = %.4f" % (
        " ".join("%.4f" % a for a in aucs), min(aucs), max(aucs) - min(aucs), 2 * min(aucs) - max(aucs)))


if __name__ == "__main__":
    main()
