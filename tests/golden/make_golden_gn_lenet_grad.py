#!/usr/bin/env python
"""Generate the GN-LeNet gradient fixtures by running the REFERENCE simulator's own model.

Run in the development container only (it needs the reference checkout, NIID_REFERENCE; the GPU
box never runs it):

    python tests/golden/make_golden_gn_lenet_grad.py

It loads theta, x and y of the two forward fixtures (tests/golden/gn_lenet/gn_lenet_{mnist,cifar}.npz,
made by make_golden_gn_lenet.py) into the reference's setup.model.gn_lenet.GN_LeNet, runs
F.nll_loss(model.forward(x), y).backward() with the 4 samples as one batch (fp32 on the CPU, a
zeroed gradient) and writes, next to them,

    tests/golden/gn_lenet/gn_lenet_mnist_grad.npz
    tests/golden/gn_lenet/gn_lenet_cifar_grad.npz

each holding
    loss   float32 []    the mean batch loss
    grad   float32 [P]   the gradients of model.parameters(), flattened in registration order

Nothing of the reference is copied into this repository: only outputs (data).
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from make_golden_gn_lenet import OUT, _gn_lenet

CASES = ("gn_lenet_mnist", "gn_lenet_cifar")


def main():
    GN_LeNet = _gn_lenet()
    for name in CASES:
        d = np.load(os.path.join(OUT, name + ".npz"))
        cin, h, w, c = (int(v) for v in d["shape"])
        model = GN_LeNet({}, input_channel=cin, output=c, model_input=(h, w))
        torch.nn.utils.vector_to_parameters(torch.from_numpy(d["theta"]), model.parameters())
        for q in model.parameters():
            q.grad = None
        loss = F.nll_loss(model.forward(torch.from_numpy(d["x"]), {}), torch.from_numpy(d["y"]))
        loss.backward()
        grad = torch.cat([q.grad.reshape(-1) for q in model.parameters()])
        assert grad.numel() == d["theta"].shape[0]
        path = os.path.join(OUT, name + "_grad.npz")
        np.savez_compressed(path, loss=loss.detach().numpy().astype(np.float32),
                            grad=grad.numpy().astype(np.float32))
        print(f"{name}: loss {loss.item():.6f}, P = {grad.numel()}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
