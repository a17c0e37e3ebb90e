"""Host-side mirror of the reference's frozen critic (critic_net.py:5-69) for the training loop:
`preds = critic.evaluate(images)` (vae.py:50).  Inference here, training in critic_train.py; parameters are kept as one flat
buffer in the reference's state_dict order (what cvae_critic_forward reads)."""
import torch
from torch import nn

from .lib import CRITIC_DECISIONS, CRITIC_EMBED_SHAPES, Handle

# reference state_dict keys, in order, with shapes (critic_net.py:15-41, default arguments)
CRITIC_KEYS = (("features.0.weight", (8, 3, 3, 3)), ("features.0.bias", (8,)),
               ("features.3.weight", (8, 8, 3, 3)), ("features.3.bias", (8,)),
               ("features.6.weight", (8, 8, 3, 3)), ("features.6.bias", (8,)),
               ("features.10.weight", (16, 8, 3, 3)), ("features.10.bias", (16,)),
               ("features.14.weight", (32, 16, 4, 4)), ("features.14.bias", (32,)),
               ("crit.1.weight", (32, 32)), ("crit.1.bias", (32,)),
               ("crit.4.weight", (1, 32)), ("crit.4.bias", (1,)))


class Critic(nn.Module):
    def __init__(self, width=64, handle=None):
        super().__init__()
        self.width = width
        self.handle = handle if handle is not None else Handle(width, 1)
        n = self.handle.lib.cvae_critic_param_count()
        assert n == sum(int(torch.tensor(s).prod()) for _, s in CRITIC_KEYS)
        self.register_buffer("flat", torch.zeros(n))

    def load_state_dict(self, sd, strict=True):
        """Accepts the reference's checkpoint (saved-networks/critic-*.pt, vae_utility.py:363-370)."""
        parts = []
        for k, shape in CRITIC_KEYS:
            t = sd[k]
            assert tuple(t.shape) == shape, (k, tuple(t.shape), shape)
            parts.append(t.reshape(-1).to(torch.float32))
        with torch.no_grad():
            self.flat.copy_(torch.cat(parts))

    def state_dict(self, *a, **k):
        out, off = {}, 0
        for key, shape in CRITIC_KEYS:
            n = int(torch.tensor(shape).prod())
            out[key] = self.flat[off:off + n].reshape(shape).clone()
            off += n
        return out

    def preprocess(self, X):
        """critic_net.py:60-63 / vae_utility.py:337-343: uint8 (B,H,W,3) -> float (B,3,H,W) / 255."""
        X = X.contiguous()
        out = torch.empty(X.shape[0], 3, self.width, self.width, device=X.device)
        self.handle.preprocess_u8(X.shape[0], X, out)
        return out

    def forward(self, X, collect=False):
        """critic_net.py:44-59 in eval mode: pred (B,1), or with collect (pred, [e1..e5]): the four pooled feature maps and
        the bottleneck (features.14 after its ReLU), as the reference's list."""
        if not collect:
            return self.evaluate(X)
        with torch.no_grad():
            X = X.to(torch.float32).contiguous()
            B = X.shape[0]
            pred = torch.empty(B, 1, device=X.device)
            embeds = [torch.empty(B, *s, device=X.device) for s in CRITIC_EMBED_SHAPES]
            self.handle.critic_collect(B, X, self.flat, pred, embeds)
        return pred, embeds

    def saliency(self, X, steps=1, return_grad=False, return_decisions=False):
        """The gradient of the critic's logit with respect to the pixels of X (B,3,64,64) in [0,1]: steps == 1 at X itself,
        steps 2..256 integrated gradients from the black frame (include/cvae.h, cvae_critic_saliency).
        -> dict(pred (B,1), map (B,64,64) grey |gradient|, max_values (B) [, grad (B,3,64,64)] [, decisions (B,11072) uint8])."""
        with torch.no_grad():
            X = X.to(torch.float32).contiguous()
            B, dev = X.shape[0], X.device
            out = {"pred": torch.empty(B, 1, device=dev), "map": torch.empty(B, 64, 64, device=dev), "max_values": torch.empty(B, device=dev)}
            if return_grad:
                out["grad"] = torch.empty(B, 3, 64, 64, device=dev)
            if return_decisions:
                out["decisions"] = torch.empty(B, CRITIC_DECISIONS, dtype=torch.uint8, device=dev)
            self.handle.critic_saliency(B, X, self.flat, steps, out["pred"], out["map"], out["max_values"], grad=out.get("grad"),
                                        decisions=out.get("decisions"))
        return out

    def occlusion(self, X, patch=8, fill=None):
        """Occlusion sensitivity (cvae_critic_occlusion): every non-overlapping patch x patch window (4, 8 or 16) of X is covered
        with the colour `fill` (three floats; None: the mean colour of X) and the critic runs again.
        -> dict(pred (B,1), drop (B,64/patch,64/patch) = pred - occluded pred, map (B,64,64) = max(drop, 0) over its patch,
        max_values (B), fill)."""
        with torch.no_grad():
            X = X.to(torch.float32).contiguous()
            B, dev, g = X.shape[0], X.device, 64 // int(patch)
            if fill is None:
                fill = X.mean(dim=(0, 2, 3)).tolist()
            fill = tuple(float(v) for v in fill)
            out = {"pred": torch.empty(B, 1, device=dev), "drop": torch.empty(B, g, g, device=dev), "map": torch.empty(B, 64, 64, device=dev),
                   "max_values": torch.empty(B, device=dev), "fill": fill}
            self.handle.critic_occlusion(B, X, self.flat, patch, fill, out["pred"], out["drop"], out["map"], out["max_values"])
        return out

    def evaluate(self, X):
        """critic_net.py:66-69: no_grad forward, returns (B,1) in (0,1)."""
        with torch.no_grad():
            X = X.to(torch.float32).contiguous()
            pred = torch.empty(X.shape[0], 1, device=X.device)
            self.handle.critic_forward(X.shape[0], X, self.flat, pred)
        return pred
