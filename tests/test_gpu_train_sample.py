"""--device-training-sample on the GPU: whole rounds of the 'sample' topology through d_sgd.init /
next_step.  The sampling equals the CPU-path plugin's; every round equals, bit for bit, the
reference's CPU arithmetic (tests/test_gpu_sample_step.py::_cpu_round) applied to the pre-round
models with the device's gradient of that round; the drift against the same rounds in float64 obeys
the rule of tests/test_gpu_train.py; the parameters stay resident between rounds.  Both ways the
trainer has of doing step + average + broadcast run: the one launch and the three ops in sequence."""
import pytest
import torch
import torch.nn.functional as F

import test_eval_gnlenet_host as th
import test_gpu_sample_step as ts

pytestmark = pytest.mark.gpu


class Linear(torch.nn.Module):
    K, C = 33, 7

    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(self.K, self.C)

    def forward(self, x, params):
        return F.log_softmax(self.fc(x.view(-1, self.K)), dim=1)


class GN(th.GNLeNet):
    def __init__(self):
        super().__init__(1, 3, (15, 15), 2)


#        model, sample shape, classes, nodes, samples per node, batch, sample size, rounds, lr
CASES = {"linear": (Linear, (33,), 7, 8, 40, 4, 3, 7, 0.1),
         "gn-lenet": (GN, (1, 15, 15), 3, 4, 12, 2, 2, 3, 0.05)}
_data = {}


def _dataset(case):
    if case not in _data:
        _, shape, c, n, s = CASES[case][:5]
        g = torch.Generator().manual_seed(77)
        if case == "linear":                    # sparse, bounded inputs: SGD at lr 0.1 is stable
            x = torch.rand(n * s, *shape, generator=g) * (torch.rand(n * s, *shape, generator=g) < 0.3)
        else:
            x = torch.randn(n * s, *shape, generator=g)
        _data[case] = (x, torch.randint(0, c, (n * s,), generator=g))
    return _data[case]


def _setup(case, flag, momentum, monkeypatch):
    from niidmix import d_sgd
    model, _, _, n, s, batch, size, _, lr = CASES[case]
    monkeypatch.setattr(d_sgd, "_sample_cache", {})       # get_sample caches node lists by step
    torch.manual_seed(2027)
    params = {"meta": {"log": "WARNING", "seed": 2027}, "nodes": {"nb-nodes": n},
              "topology": {"name": "sample", "sample-method": "random-with-overlap", "sample-size": size,
                           "sample-overlap": 1},
              "logger": {"accuracy-logging-interval": 0, "accuracy-logging-interval-steps": 0,
                         "log-consensus-distance": False},
              "algorithm": {"learning-rate": lr, "learning-momentum": momentum, "batch-size": batch,
                            "initial-averaging": False, "clique-gradient": False,
                            "unbiased-gradient": False, "deferred-writeback": False,
                            "mixing-mode": "exact"}}
    if flag:
        params["algorithm"].update({"device-training": True, "device-training-sample": True})
        if case == "gn-lenet":
            params["algorithm"]["device-training-gn-lenet"] = True
    x, y = _dataset(case)
    gen = torch.Generator().manual_seed(2028)
    nodes = []
    for r in range(n):
        mdl = model()
        if case == "gn-lenet":
            th.perturb(mdl, gen)
        nodes.append({"rank": r, "epoch": 0, "model": mdl, "optimizer": d_sgd.optimizer(mdl, params),
                      "train-set": [(x[r * s + j], int(y[r * s + j])) for j in range(s)]})
    state, _, _ = d_sgd.init(nodes, {"edges": {}, "weights": []}, params)
    return params, nodes, state


def _flat(nodes):
    return torch.stack([torch.cat([q.detach().reshape(-1) for q in nd["model"].parameters()])
                        for nd in nodes]).clone()


def _run(case, flag, momentum, monkeypatch):
    """The plugin's rounds; with the flag, every round is checked against the CPU restatement on
    the device's own gradients.  Returns (final models, [(active ranks, loss keys, epoch_done)],
    RNG state, the trainer or None)."""
    from niidmix import d_sgd
    params, nodes, state = _setup(case, flag, momentum, monkeypatch)
    lr, rounds = CASES[case][8], CASES[case][7]
    buf = torch.zeros_like(_flat(nodes))
    stepped, log, tr = set(), [], None
    for k in range(rounds):
        pre = _flat(nodes)
        state, losses, done, active = d_sgd.next_step(state, params, None)
        d_sgd.synchronize()
        ranks = [nd["rank"] for nd in active]
        log.append((ranks, sorted(losses), done))
        assert sorted(done) == sorted(ranks) and all(isinstance(v, float) for v in losses.values())
        if flag:
            tr = d_sgd._trainers[id(nodes)]
            first = [r not in stepped for r in ranks]
            assert tr.last_first == [int(f) for f in first], f"round {k}"
            stepped.update(ranks)
            grad = torch.zeros_like(pre)
            grad[ranks] = tr.grad[ranks].cpu()
            want, buf = ts._cpu_round(pre, grad, buf, ranks, first, momentum, lr)
            got = _flat(nodes)
            assert ts._same_bits(got, want), f"round {k}"
            assert bool((got == got[0]).all())                   # finite models: every row the average
            if momentum:
                assert ts._same_bits(tr.mbuf.cpu(), buf), f"round {k}"
    assert state["step"] == rounds
    return _flat(nodes), log, torch.get_rng_state(), tr, (params, nodes, state)


def _fp64_rounds(case, momentum, monkeypatch):
    """The same rounds in float64: the same samples and batches, the family's float64 gradient."""
    from niidmix import d_sgd, train
    params, nodes, state = _setup(case, True, momentum, monkeypatch)
    _, shape, c, n, s, _, _, rounds, lr = CASES[case]
    x, y = _dataset(case)
    th64 = _flat(nodes).double()
    buf = {}
    for k in range(rounds):
        active = d_sgd.get_sample(state, params, k)
        batches, _ = train.draw(active, params)
        new = []
        for nd, idx in zip(active, batches):
            r = nd["rank"]
            xb, yb = x[idx + r * s], y[idx + r * s]
            if case == "linear":
                kk = shape[0]
                _, g, _ = train.fp64_reference(th64[r, :c * kk].view(c, kk), th64[r, c * kk:], xb, yb)
            else:
                _, g = train.fp64_reference_gn_lenet(th64[r], xb, yb)
            if momentum:
                g = buf[r] = momentum * buf[r] + g if r in buf else g.clone()
            new.append(th64[r] - lr * g)
        th64 = (sum(new) / len(new)).expand(n, -1).clone()
    return th64


@pytest.mark.parametrize("path", ["one launch", "three ops"])
@pytest.mark.parametrize("case,momentum", [("linear", 0.0), ("linear", 0.9), ("gn-lenet", 0.9)])
def test_rounds_against_the_cpu_path(gpu, monkeypatch, case, momentum, path):
    from niidmix import train
    monkeypatch.setattr(train, "SAMPLE_FUSED_MIN_COLS", 0 if path == "one launch" else 1 << 40)
    monkeypatch.setattr(train, "SAMPLE_FUSED_MIN_SHARE", 0.0)
    th_c, log_c, rng_c, tr, _ = _run(case, True, momentum, monkeypatch)
    assert tr.sample and tr.sample_fused == (path == "one launch") and tr.mixer is None
    assert tr.param_uploads == 1                                  # resident between the rounds
    th_a, log_a, rng_a, _, _ = _run(case, False, momentum, monkeypatch)
    assert log_c == log_a                                        # active ranks, loss keys, epoch_done
    assert torch.equal(rng_c, rng_a)
    assert len({tuple(r) for r, _, _ in log_c}) > 1              # the sample moves
    th_b = _fp64_rounds(case, momentum, monkeypatch)
    drift_a = float((th_a.double() - th_b).abs().max())
    drift_c = float((th_c.double() - th_b).abs().max())
    print(f"{case} m={momentum} {path}: max|theta_a - theta_b| {drift_a:.3g}  "
          f"max|theta_c - theta_b| {drift_c:.3g}")
    assert drift_c <= 10 * drift_a


def test_parameters_stay_resident_for_readers(gpu, monkeypatch):
    """After a round tr.current() is the device slab (what --device-evaluation reads in place), and
    the next round uploads nothing; a write behind the plugin's back is uploaded again."""
    from niidmix import d_sgd
    _, _, _, tr, (params, nodes, state) = _run("linear", True, 0.9, monkeypatch)
    cur = tr.current()
    assert cur is not None and torch.equal(cur.cpu().view(torch.int32), _flat(nodes).view(torch.int32))
    got = d_sgd.device_trainer([nd["model"] for nd in nodes[2:5]])
    assert got is not None and got[0] is tr and got[1] == [2, 3, 4]
    uploads = tr.param_uploads
    state, _, _, _ = d_sgd.next_step(state, params, None)
    assert tr.param_uploads == uploads and tr.current() is not None
    with torch.no_grad():
        nodes[1]["model"].fc.bias.data.add_(1)
    d_sgd.invalidate([nodes[1]])
    assert tr.current() is None
    d_sgd.next_step(state, params, None)
    assert tr.param_uploads == uploads + 1
