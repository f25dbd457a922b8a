"""Generate tests/golden/opacity_loss.npz by running the REFERENCE's mask-supervision losses:
LitNeRF_AutoDecoder.opacity_loss / opacity_loss_CE / opacity_loss_autorf
(models/vanilla_nerf/model_autodecoder.py:703-766; none of them touches ``self``, so they are
called unbound with None) and the foreground-only colour loss img2mse(rgb[mask], target[mask])
(model_autodecoder.py:423-426), in fp32 on the CPU, with their autograd gradients.

Runs only where the reference tree is present (see _refimport.py); the fixture is data only.

    python tests/golden/make_golden_opacity.py

Per case NAME the file holds NAME__acc0 / acc1 (B) fp32, NAME__mask (B) uint8, for every KIND in
mse / ce / autorf NAME__KIND_loss (fp32 scalar) and NAME__KIND_g0 / _g1 (d loss / d acc0, acc1),
and for the masked-colour cases NAME__pred0 / pred1 / target (B,3), NAME__rgb_loss0 / rgb_loss1
and NAME__rgb_g0 / rgb_g1.  ``cases`` lists the names, ``rgb_cases`` those with colours.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _refimport  # noqa: E402

# (name, B, mask: Bernoulli probability of foreground, masked-colour case)
CASES = [("b1", 1, 0.4, False), ("b255", 255, 0.4, False), ("b256", 256, 0.4, False),
         ("b257", 257, 0.4, False), ("b2047", 2047, 0.4, False), ("b2049", 2049, 0.4, False),
         ("b300_bg", 300, 0.0, False), ("b300_fg", 300, 1.0, False),
         ("b300_rgb", 300, 0.4, True), ("b64_rgb_bg", 64, 0.0, True)]


def main():
    mad = _refimport.load_articulated()
    helper = sys.modules["models.vanilla_nerf.helper"]
    lit = mad.LitNeRF_AutoDecoder
    kinds = {"mse": lit.opacity_loss, "ce": lit.opacity_loss_CE, "autorf": lit.opacity_loss_autorf}
    torch.set_num_threads(1)
    out = {"cases": np.array([c[0] for c in CASES]),
           "rgb_cases": np.array([c[0] for c in CASES if c[3]])}
    for k, (name, B, p_fg, rgb) in enumerate(CASES):
        rng = np.random.Generator(np.random.PCG64(1000 + k))
        acc = [(rng.random(B, dtype=np.float32) * np.float32(1.2) - np.float32(0.1))
               for _ in range(2)]  # uniform in [-0.1, 1.1): the clamp has work to do
        mask = rng.random(B) < p_fg
        out[f"{name}__acc0"], out[f"{name}__acc1"] = acc
        out[f"{name}__mask"] = mask.astype(np.uint8)
        m = torch.from_numpy(mask)
        for kind, fn in kinds.items():
            a0, a1 = (torch.from_numpy(a).clone().requires_grad_(True) for a in acc)
            loss = fn(None, [(None, a0), (None, a1)], m)
            loss.backward()
            out[f"{name}__{kind}_loss"] = loss.detach().numpy().astype(np.float32)
            for i, a in enumerate((a0, a1)):
                g = a.grad if a.grad is not None else torch.zeros_like(a)
                out[f"{name}__{kind}_g{i}"] = g.numpy()
        if rgb:
            target = rng.random((B, 3), dtype=np.float32)
            out[f"{name}__target"] = target
            m3 = m.view(-1, 1).repeat(1, 3)  # model_autodecoder.py:423
            for i in range(2):
                pred = rng.random((B, 3), dtype=np.float32)
                p = torch.from_numpy(pred).clone().requires_grad_(True)
                loss = helper.img2mse(p[m3], torch.from_numpy(target)[m3])
                loss.backward()
                out[f"{name}__pred{i}"] = pred
                out[f"{name}__rgb_loss{i}"] = loss.detach().numpy().astype(np.float32)
                out[f"{name}__rgb_g{i}"] = p.grad.numpy()
    path = os.path.join(HERE, "opacity_loss.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
