"""One side of the training-rate comparison: builds a 50 000-entry dataset, then times one fit_device epoch per 'go' line."""
import sys, time
import numpy as np, torch
side, prec, B = sys.argv[1], sys.argv[2], int(sys.argv[3])
from critic_vae_amd import episodes as E
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.train import FusedTrainer
dev = torch.device("cuda:0")
N = 50000
g = torch.Generator(device=dev); g.manual_seed(1)
if side == "recon":
    frames = torch.empty(N, 3, 64, 64, device=dev)
    for p in range(0, N, 5000):
        frames[p:p + 5000] = torch.rand(5000, 3, 64, 64, device=dev, generator=g) * 1.6 - 0.8
    ds = E.ReconDataset(frames, torch.rand(N, 1, device=dev, generator=g), np.zeros((N, 3), np.int64))
else:
    frames = torch.randint(0, 256, (N, 64, 64, 3), dtype=torch.uint8, device=dev, generator=g)
    ds = E.DeviceDataset(frames, torch.rand(N, 1, device=dev, generator=g), np.zeros((N, 2), np.int64))
vae = VariationalAutoencoder(max_batch=B, seed=5, precision=prec).to(dev)
tr = FusedTrainer(vae)
np.random.seed(0)
tr.fit_device(ds, B, epochs=1, generator=g)          # warm-up epoch
torch.cuda.synchronize()
print("ready", flush=True)
for line in sys.stdin:
    if line.strip() != "go":
        break
    torch.cuda.synchronize(); t0 = time.perf_counter()
    tr.fit_device(ds, B, epochs=1, generator=g)
    torch.cuda.synchronize()
    print(f"{N / (time.perf_counter() - t0):.1f}", flush=True)
