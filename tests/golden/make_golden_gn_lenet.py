#!/usr/bin/env python
"""Generate the GN-LeNet fixtures by running the REFERENCE simulator's own model.

Run in the development container only (it needs the reference checkout, NIID_REFERENCE; the GPU
box never runs it):

    python tests/golden/make_golden_gn_lenet.py

It builds the reference's setup.model.gn_lenet.GN_LeNet (with make_golden.py's empty torchvision
stub: the model's import chain reaches setup.dataset, which imports torchvision for datasets
only), perturbs every bias and GroupNorm affine parameter away from its 0 / 1 default, runs
model.forward on 4 random samples and writes, per shape,

    tests/golden/gn_lenet/gn_lenet_mnist.npz    Cin 1, 28 x 28, C 10  (P = 80554)
    tests/golden/gn_lenet/gn_lenet_cifar.npz    Cin 3, 32 x 32, C 10  (P = 85354)

(in a directory of their own: every *.npz directly under tests/golden/ is taken for a mixing
fixture by conftest.golden_cases), each holding
    shape     int64 [4]      Cin, H, W, C
    theta     float32 [P]    model.parameters() flattened in registration order
    x         float32 [4, Cin, H, W]
    y         int64 [4]
    logprobs  float32 [4, C] the reference's forward (log_softmax of the classifier), fp32 on the CPU

Nothing of the reference is copied into this repository: only inputs and outputs (data).
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("NIID_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gn_lenet")
CASES = {"gn_lenet_mnist": (1, 28, 28, 10, 101), "gn_lenet_cifar": (3, 32, 32, 10, 102)}


def _gn_lenet():
    for name in ["torchvision", "torchvision.datasets", "torchvision.transforms", "torchvision.utils"]:
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].datasets = sys.modules["torchvision.datasets"]
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.path.insert(0, os.path.join(REF, "tools"))
    import importlib
    return importlib.import_module("setup.model.gn_lenet").GN_LeNet


def main():
    GN_LeNet = _gn_lenet()
    os.makedirs(OUT, exist_ok=True)
    for name, (cin, h, w, c, seed) in CASES.items():
        torch.manual_seed(seed)
        model = GN_LeNet({}, input_channel=cin, output=c, model_input=(h, w))
        gen = torch.Generator().manual_seed(seed + 1000)
        with torch.no_grad():
            for q in model.parameters():
                if q.dim() == 1:             # biases and GroupNorm affines: off their 0 / 1 defaults
                    q.add_(0.2 * torch.randn(q.shape, generator=gen))
        x = torch.randn(4, cin, h, w, generator=gen)
        y = torch.randint(0, c, (4,), generator=gen)
        with torch.no_grad():
            lp = model.forward(x, {})
        theta = torch.cat([q.detach().reshape(-1) for q in model.parameters()])
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, shape=np.array([cin, h, w, c], np.int64), theta=theta.numpy(),
                            x=x.numpy(), y=y.numpy(), logprobs=lp.numpy())
        print(f"{name}: P = {theta.numel()}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
