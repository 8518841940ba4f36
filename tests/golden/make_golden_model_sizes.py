#!/usr/bin/env python3
"""Golden vectors for the model-size ladders (reference train_model.py:337-370), recorded by
BUILDING the upstream reference's own models in the build container.

    python tests/golden/make_golden_model_sizes.py        (needs /root/reference)

For every ``args.model`` name of the two ladders that ``build_model`` accepts beyond 'Potes' and
'resnet9', the reference's factory is called exactly as its dispatcher calls it (num_channels 4,
num_classes 2, dataset 'PhysioNet') under ``torch.manual_seed(11)``, put in eval mode and run on
``x = RandomState(3).randn(3, 4, 2500)`` in float32.

Written to tests/golden/model_sizes.npz (only data: no weights, no reference source):

  names           the args.model names, in order
  params          number of parameters of each model (all of them, trainable or not)
  logits          (len(names), 3, 2) float32 logits of ``model(x)``
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from _ref_import import import_reference  # noqa: E402

SEED, X_SEED, X_SHAPE = 11, 3, (3, 4, 2500)


def reference_builders(M):
    """args.model -> the call the reference's dispatcher makes (train_model.py:341-370)."""
    kw = dict(num_channels=4, num_classes=2)
    res = dict(in_channels=4, num_classes=2)
    return {
        "Potes0.02": lambda: M.CNN_potes_twopercent_TS(**kw),
        "Potes0.1": lambda: M.CNN_potes_tenpercent_TS(**kw),
        "Potes(noDropout)": lambda: M.CNN_potes_TS(dataset="PhysioNet", dropout=0.0, **kw),
        "PotesBig64and32": lambda: M.CNN_potes_big64and32_TS(dataset="PhysioNet", **kw),
        "PotesBig128and64": lambda: M.CNN_potes_big128and64_TS(dataset="PhysioNet", **kw),
        "resnet9-5k": lambda: M.ResNet9(filters=[2, 4, 8, 16], linear=1248, **res),
        "resnet9-15k": lambda: M.ResNet9(filters=[4, 8, 16, 32], linear=2496, **res),
        "resnet9-50k": lambda: M.ResNet9(filters=[8, 16, 32, 64], linear=4992, **res),
        "resnet9-150k": lambda: M.ResNet9(filters=[16, 32, 64, 128], linear=9984, **res),
        "resnet9-600k": lambda: M.ResNet9(filters=[32, 64, 128, 256], linear=19968, **res),
        "resnet9-1.4m": lambda: M.ResNet9(filters=[64, 128, 192, 384], linear=29952, **res),
        "resnet9-2.3m": lambda: M.ResNet9(filters=[64, 128, 256, 512], linear=39936, **res),
        "resnet9-5m": lambda: M.ResNet9(filters=[96, 192, 384, 768], linear=59904, **res),
        "resnet9-9m": lambda: M.ResNet9(filters=[128, 256, 512, 1024], linear=79872, **res),
    }


def main():
    ref = import_reference()
    x = torch.from_numpy(np.random.RandomState(X_SEED).randn(*X_SHAPE).astype(np.float32))
    names, params, logits = [], [], []
    for name, build in reference_builders(ref.models).items():
        torch.manual_seed(SEED)
        m = build().eval()
        with torch.no_grad():
            out = m(x)
        names.append(name)
        params.append(sum(p.numel() for p in m.parameters()))
        logits.append(out.numpy().astype(np.float32))
        print(f"{name:18s} {params[-1]:9d}  {logits[-1][0]}")
    path = os.path.join(HERE, "model_sizes.npz")
    np.savez(path, names=np.array(names), params=np.array(params, dtype=np.int64),
             logits=np.stack(logits))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
