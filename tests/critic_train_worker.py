"""Child process of tests/test_gpu_critic_train.py: one cvae_critic_grad call at B = 37 on the fixture's inputs, started
fresh with CVAE_PERSIST_MAXWG in its environment (the library reads the cap once per process), results to an .npz.

    python tests/critic_train_worker.py OUT.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main(out):
    import critic_train_tools as T
    fx = T.load_fixture(os.path.join(HERE, "golden"))
    z = fx["z"]
    res = {}
    for loss in ("bce", "mse"):
        r = T.run_kernel(T.make_handle(), fx["flat"], fx["x"], z["target"], z["keep"], float(z["dropout_p"]), loss)
        for k in ("grads", "pred", "scalars", "decisions", "partials_written"):
            res[f"{loss}/{k}"] = r[k]
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
