"""Child process of tests/test_gpu_critic_saliency.py: B = 37 real frames through cvae_critic_saliency (steps 1 and 3),
cvae_critic_occlusion (P = 8) and cvae_critic_collect, started fresh with CVAE_PERSIST_MAXWG in its environment (the library
reads the cap once per process), results to an .npz.

    python tests/critic_saliency_worker.py OUT.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

B, FILL = 37, (0.25, 0.5, 0.125)


def run_all(S, h, fx, x):
    res = {}
    for steps in (1, 3):
        r = S.run_saliency(h, fx["flat"], x, steps)
        for k, v in r.items():
            res[f"sal{steps}/{k}"] = v
    for k, v in S.run_occlusion(h, fx["flat"], x, 8, FILL).items():
        res[f"occ/{k}"] = v
    for k, v in S.run_collect(h, fx["flat"], x).items():
        res[f"col/{k}"] = v
    return res


def main(out):
    import critic_saliency_tools as S
    import critic_train_tools as T
    fx = S.load_fixture(os.path.join(HERE, "golden"))
    h = T.make_handle()
    res = run_all(S, h, fx, fx["x"][:B])
    # the cap's witness: cvae_critic_grad sizes its grid with the same helper and leaves one partial per workgroup in scratch
    res["workgroups"] = T.run_kernel(h, fx["flat"], fx["x"][:B], np.zeros(B, np.float32), None, 0.0, "bce")["partials_written"]
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
