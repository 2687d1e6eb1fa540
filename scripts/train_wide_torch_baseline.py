"""The Wide&Deep learning test's thresholds (tests/test_train_wide.py::test_it_learns_what_only_the_cross_carries): torch.optim.Adam(eps=1e-7)
on the CPU, on the graph and the exact arrays of tests/train_wide_cases.py (learning(): labels a function of the cross bucket, hidden (2,),
batch 256, 10 epochs, lr 0.02), over five initialisation seeds and both cross forms.  Prints per seed the final mean training loss, then
worst + (worst - best): the threshold the test uses.

    python scripts/train_wide_torch_baseline.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests import train_wide_cases as TWC
    for cross_dim in (0, 3):
        losses = []
        for seed in range(5):
            fam, w, ids, dense, y = TWC.learning(cross_dim, seed)
            losses.append(TWC.torch_adam_fit(fam, w, ids, dense, y, 256, 10, 0.02))
        print("cross_dim %d: final losses %s; worst %.4f, spread %.4f, threshold = worst + spread = %.4f" % (
            cross_dim, " ".join("%.4f" % l for l in losses), max(losses), max(losses) - min(losses), 2 * max(losses) - min(losses)))


if __name__ == "__main__":
    main()
