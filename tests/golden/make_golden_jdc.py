"""Generates tests/golden/jdc.npz and tests/golden/jdc_state_shapes.json by importing the REAL reference's F0 extractor
(modules/JDC/model.py, build container only, like make_golden.py): JDCNet(num_class=1, seq_len=192) as modules/commons.py:186
builds it, in .eval(), with synth.synth_jdc_state_dict(0) loaded.

Run:  python tests/golden/make_golden_jdc.py            (seconds)

Inputs (stored): x0 (2, 1, 80, 24) and x1 (3, 1, 80, 17), standard normal from a seeded generator.
Per input i: F0_i (B, T); gan_i = every 8th channel of GAN_feature (B, 256, 10, T); pool_i = every 8th channel of poolblock_out
(B, 256, T, 2); and err_F0_i / err_gan_i / err_pool_i, the reference's own fp32-against-fp64 error relative to max |fp64| of each.
`forward` calls x.float(), so the fp64 run walks the submodules of a .double() copy in the order of model.py:111-137; the same walk
in fp32 is asserted bit-equal to `forward`.

jdc_state_shapes.json: {key: [shape, dtype]} of the reference's state dict.  Both files are data only."""
import copy
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)

from facodec_amd import synth  # noqa: E402


def ref_jdc():
    spec = importlib.util.spec_from_file_location("ref_jdc_model", os.path.join(REF, "modules", "JDC", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.JDCNet


def walk(m, x):
    """model.py:111-137 through m's submodules in x's dtype -> (F0, GAN_feature, poolblock_out)."""
    seq_len = x.shape[-1]
    h = x.transpose(-1, -2)
    h = m.res_block3(m.res_block2(m.res_block1(m.conv_block(h))))
    h = m.pool_block[1](m.pool_block[0](h))
    gan = h.transpose(-1, -2)
    pooled = m.pool_block[2](h)
    c = pooled.permute(0, 2, 1, 3).contiguous().view((-1, seq_len, 512))
    c, _ = m.bilstm_classifier(c)
    c = m.classifier(c.contiguous().view((-1, 512))).view((-1, seq_len, m.num_class))
    return torch.abs(c.squeeze(-1)), gan, pooled


def rel(a, b64):
    return float((a.double() - b64).abs().max() / b64.abs().max())


def main():
    torch.manual_seed(0)
    JDCNet = ref_jdc()
    model = JDCNet(num_class=1, seq_len=192).eval()
    shapes = {k: (tuple(v.shape), v.dtype) for k, v in model.state_dict().items()}
    model.load_state_dict(synth.synth_jdc_state_dict(0, shapes), strict=True)
    model64 = copy.deepcopy(model).double().eval()
    g = torch.Generator().manual_seed(20240)
    out = {}
    with torch.no_grad():
        for i, shp in enumerate(((2, 1, 80, 24), (3, 1, 80, 17))):
            x = torch.randn(*shp, generator=g)
            got = model(x)
            again = walk(model, x)
            assert all(torch.equal(a, b) for a, b in zip(got, again)), "the submodule walk is not the reference's forward"
            ref64 = walk(model64, x.double())
            assert got[0].shape == shp[::3] and got[1].shape == (shp[0], 256, 10, shp[3]) and got[2].shape == (shp[0], 256, shp[3], 2)
            out[f"x{i}"] = x.numpy()
            out[f"F0_{i}"] = got[0].numpy()
            out[f"gan_{i}"] = got[1][:, ::8].contiguous().numpy()
            out[f"pool_{i}"] = got[2][:, ::8].contiguous().numpy()
            for name, a, b in zip(("F0", "gan", "pool"), got, ref64):
                out[f"err_{name}_{i}"] = np.float64(rel(a, b))
            print(shp, "F0 range", float(got[0].min()), float(got[0].max()),
                  {n: float(out[f"err_{n}_{i}"]) for n in ("F0", "gan", "pool")})
    np.savez_compressed(os.path.join(HERE, "jdc.npz"), **out)
    with open(os.path.join(HERE, "jdc_state_shapes.json"), "w") as f:
        json.dump({k: [list(s), str(d).replace("torch.", "")] for k, (s, d) in shapes.items()}, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
