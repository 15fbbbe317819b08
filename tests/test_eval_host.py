"""--device-evaluation, the parts that need no GPU: the C entry point's argument checks, the
scratch size, the 1000-chunking and its folding, the events the replaced Logger.state writes (with
a stubbed evaluator and a stand-in simulate.logger), the flag and its refusals."""
import json
import os
import re
import sys
import types

import pytest
import torch

from conftest import REPO


class Net(torch.nn.Module):
    def __init__(self, k=6, c=3):
        super().__init__()
        self.fc = torch.nn.Linear(k, c)

    def forward(self, x, params):
        return torch.nn.functional.log_softmax(self.fc(x.view(-1, self.fc.in_features)), dim=1)


class Net3(Net):
    def __init__(self):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.ones(1))


def test_eval_argument_errors_without_gpu():
    """Validation happens before any HIP call, in the order include/niidmix.h documents; the
    made-up addresses are never dereferenced."""
    from niidmix import _lib
    L = _lib.lib
    F = L.niidmix_linear_eval_rows_f32
    B = L.niidmix_linear_eval_rows_scratch_bytes
    base, far, scr = 1 << 20, 1 << 30, 1 << 40
    k, c, n, ml = 5, 3, 2, 100
    p = c * k + c

    def call(theta=base, ld_t=p, data=8, labels=8, rows=8, start=8, length=8, n_jobs=n, max_len=ml,
             loss=far, correct=far + 4096, pred=None, ld_pred=0, K=k, C=c, scratch=scr, nbytes=None):
        if nbytes is None:
            nbytes = B(max(n_jobs, 1), max(max_len, 0), max(C, 1))
        return F(theta, ld_t, data, labels, rows, start, length, n_jobs, max_len, loss, correct, pred,
                 ld_pred, K, C, scratch, nbytes, None)

    def err():
        return L.niidmix_last_error()

    for name in ("theta", "data", "labels", "rows", "start", "length", "loss", "correct", "scratch"):
        assert call(**{name: None}) == _lib.EINVAL and b"null" in err(), name
    for name in ("n_jobs", "K", "C"):
        for v in (0, -1):
            assert call(**{name: v}) == _lib.EINVAL and b">= 1" in err(), name
    assert call(max_len=-1) == _lib.EINVAL and b"max_len" in err()
    assert call(n_jobs=0, theta=None) == _lib.EINVAL and b"null" in err()          # null before sizes
    assert call(C=1025, ld_t=1025 * k + 1025) == _lib.EUNSUPPORTED and b"C 1025" in err()
    assert call(K=(1 << 20) + 1, ld_t=c * ((1 << 20) + 1) + c) == _lib.EUNSUPPORTED
    assert call(K=0, C=1025) == _lib.EINVAL                                       # sizes before limits
    assert call(C=1025, ld_t=1) == _lib.EUNSUPPORTED                              # limits before ld
    assert call(ld_t=p - 1) == _lib.EINVAL and b"leading dimension < C * K + C" in err()
    assert call(pred=far + 8192, ld_pred=ml - 1) == _lib.EINVAL and b"ld_pred" in err()
    assert call(ld_t=p - 1, pred=far + 8192, ld_pred=ml - 1) == _lib.EINVAL and b"leading" in err()
    assert call(nbytes=1) == _lib.EINVAL and b"scratch" in err()
    assert call(scratch=scr + 4) == _lib.EINVAL and b"scratch" in err()           # 8-B alignment
    assert call(pred=far + 8192, ld_pred=ml - 1, nbytes=1) == _lib.EINVAL and b"ld_pred" in err()
    assert call(loss=base) == _lib.EALIAS and b"overlaps theta" in err()
    assert call(correct=base + 4 * (p - 1)) == _lib.EALIAS
    assert call(pred=base - 4 * ml, ld_pred=ml) == _lib.EALIAS                    # its second row
    assert call(scratch=base + 8) == _lib.EALIAS
    assert call(loss=base, nbytes=1) == _lib.EINVAL                               # scratch before alias


def test_eval_scratch_bytes_is_monotone():
    from niidmix import _lib
    B = _lib.lib.niidmix_linear_eval_rows_scratch_bytes
    assert B(0, 10, 3) == 0 and B(5, 0, 3) == 0 and B(5, 10, 0) == 0
    assert B(1, 1, 1) >= 12
    for n, m, c in [(1, 1, 1), (7, 63, 10), (7, 64, 10), (7, 65, 10), (1000, 10000, 10), (3, 257, 1024)]:
        assert B(n, m, c) % 16 == 0 and B(n, m, c) >= 12 * n * ((m + 63) // 64)
        assert B(n + 1, m, c) >= B(n, m, c)
        assert B(n, m + 1, c) >= B(n, m, c) and B(n, m + 64, c) > B(n, m, c)
        assert B(n, m, c + 1) >= B(n, m, c)


def test_header_declares_the_eval_symbols_at_abi_6():
    from niidmix import _lib
    assert _lib.lib.niidmix_abi_version() == 6
    text = open(os.path.join(REPO, "include", "niidmix.h")).read()
    assert re.search(r"^int niidmix_linear_eval_rows_f32\(", text, re.M)
    assert re.search(r"^int64_t niidmix_linear_eval_rows_scratch_bytes\(", text, re.M)
    assert "NOT checked by the launcher" in text
    assert "niidmix_linear_eval_rows_f32" in _lib.SIGNATURES


def test_chunk_jobs_and_fold():
    """Nodes of 2500, 1000, 3 and 0 samples: consecutive chunks of 1000, the last one short; the
    loss is the mean of the chunks' means (not the mean over samples), the accuracy total correct
    over total samples."""
    from niidmix import evaluate
    node, start, length = evaluate.chunk_jobs([0, 2500, 3500, 3503, 3503])
    assert node == [0, 0, 0, 1, 2]
    assert start == [0, 1000, 2000, 2500, 3500]
    assert length == [1000, 1000, 500, 1000, 3]
    loss_sum = [2000.0, 1000.0, 250.0, 700.0, 6.0]
    correct = [900, 800, 100, 1000, 0]
    res = evaluate.fold_chunks(4, node, length, loss_sum, correct)
    assert res[0] == (1800 / 2500, (2.0 + 1.0 + 0.5) / 3)        # by samples: 3250 / 2500 = 1.3
    assert res[1] == (1.0, 0.7)
    assert res[2] == (0.0, 2.0)
    assert res[3] == (0.0, 0.0)
    assert evaluate.chunk_jobs([5, 5]) == ([], [], [])


class _StubEvaluator:
    """accuracy / train_accuracy with made-up numbers; records the calls."""

    def __init__(self):
        self.calls = []

    def train_accuracy(self, nodes):
        self.calls.append(("train", [n["rank"] for n in nodes]))
        return [(0.5 + 0.01 * n["rank"], 1.0 + n["rank"]) for n in nodes]

    def accuracy(self, items, name):
        ranks = [it["rank"] if isinstance(it, dict) else "center" for it in items]
        self.calls.append((name, ranks))
        base = {"test": 0.1, "valid": 0.2, "full-train": 0.3}[name]
        return [(base + (0.001 * r if r != "center" else 0.05), 10 * base) for r in ranks]


def _fake_logger(monkeypatch, tmp_path, **logger_params):
    lg = types.ModuleType("simulate.logger")

    class Logger:
        def __init__(self, params, rundir):
            self.params, self.rundir = params, rundir
            n = params["nodes"]["nb-nodes"]
            self.running_loss = [0.0] * n
            self.running_loss_count = [0] * n
            self.global_events = os.path.join(rundir, "events", "global.jsonlines")

        def state(self, nodes, state):
            raise AssertionError("the reference's ssh version")

        def log_consensus_distance(self, state):
            raise AssertionError("reference CPU version")
    lg.Logger = Logger
    monkeypatch.setitem(sys.modules, "simulate.logger", lg)
    lp = {"skip-training": False, "skip-testing": False, "skip-validation": False,
          "skip-full-training": False, "log-global-model-accuracy": False}
    lp.update(logger_params)
    params = {"nodes": {"nb-nodes": 4}, "logger": lp, "algorithm": {"device-evaluation": True}}
    (tmp_path / "events").mkdir()
    logger = Logger(params, str(tmp_path))
    nodes = [{"rank": r, "epoch": 2, "model": Net(),
              "event-file": str(tmp_path / "events" / f"{r}.jsonlines")} for r in (1, 3)]
    return logger, nodes, params


NODE_KEYS = ["type", "data", "rank", "epoch", "step", "loss", "accuracy", "timestamp"]
TRAIN_KEYS = ["type", "data", "rank", "epoch", "step", "loss", "running_loss", "accuracy", "timestamp"]
GLOBAL_KEYS = ["type", "data", "epoch", "step", "loss", "accuracy", "timestamp"]


def test_state_events_and_running_loss(monkeypatch, tmp_path):
    """Two logged nodes (ranks 1 and 3): the train events carry the mean of the collected losses
    and reset the bookkeeping as Logger.log_train_accuracy does; the test / valid / full-train
    events follow, one evaluator call per set for all nodes."""
    from niidmix import logger as nl
    logger, nodes, _ = _fake_logger(monkeypatch, tmp_path)
    logger.running_loss[1], logger.running_loss_count[1] = 6.0, 4
    logger.running_loss[3], logger.running_loss_count[3] = 5.0, 0       # a sum without a count stays
    ev = _StubEvaluator()
    out = nl.state_events(ev, logger, nodes, {"step": 7})
    assert ev.calls == [("train", [1, 3]), ("test", [1, 3]), ("valid", [1, 3]), ("full-train", [1, 3])]
    files = [os.path.basename(p) for p, _ in out]
    assert files == ["1.jsonlines", "3.jsonlines"] + ["1.jsonlines"] * 3 + ["3.jsonlines"] * 3
    t1, t3 = out[0][1], out[1][1]
    assert list(t1) == TRAIN_KEYS
    assert (t1["data"], t1["rank"], t1["epoch"], t1["step"]) == ("train", 1, 2, 7)
    assert (t1["accuracy"], t1["loss"], t1["running_loss"]) == (0.5 + 0.01 * 1, 2.0, 6.0 / 4)
    assert (t3["accuracy"], t3["loss"], t3["running_loss"]) == (0.5 + 0.01 * 3, 4.0, 0.0)
    assert logger.running_loss == [0.0, 0.0, 0.0, 5.0] and logger.running_loss_count == [0, 0, 0, 0]
    rest = [e for _, e in out[2:]]
    assert [(e["rank"], e["data"]) for e in rest] == [(1, "test"), (1, "valid"), (1, "full-train"),
                                                      (3, "test"), (3, "valid"), (3, "full-train")]
    assert all(list(e) == NODE_KEYS and e["type"] == "accuracy" and e["step"] == 7 for e in rest)
    assert (rest[0]["accuracy"], rest[0]["loss"]) == (0.1 + 0.001 * 1, 10 * 0.1)
    assert (rest[5]["accuracy"], rest[5]["loss"]) == (0.3 + 0.001 * 3, 10 * 0.3)
    # a second state without new losses: running_loss 0.0
    out = nl.state_events(ev, logger, nodes, {"step": 8})
    assert out[0][1]["running_loss"] == 0.0 and out[0][1]["step"] == 8


def test_state_events_skip_flags(monkeypatch, tmp_path):
    from niidmix import logger as nl
    logger, nodes, _ = _fake_logger(monkeypatch, tmp_path, **{"skip-training": True,
                                                               "skip-validation": True})
    logger.running_loss[1], logger.running_loss_count[1] = 6.0, 4
    ev = _StubEvaluator()
    out = nl.state_events(ev, logger, nodes, {"step": 1})
    assert ev.calls == [("test", [1, 3]), ("full-train", [1, 3])]
    assert [(e["rank"], e["data"]) for _, e in out] == [(1, "test"), (1, "full-train"),
                                                        (3, "test"), (3, "full-train")]
    assert logger.running_loss[1] == 6.0 and logger.running_loss_count[1] == 4    # untouched
    logger.params["logger"].update({"skip-testing": True, "skip-full-training": True})
    ev = _StubEvaluator()
    assert nl.state_events(ev, logger, nodes, {"step": 2}) == [] and ev.calls == []


def test_state_events_global_model(monkeypatch, tmp_path):
    """log-global-model-accuracy: train (on the full train set), test, valid of the average of the
    logged nodes' models, without a rank, in global.jsonlines; inconsistent epochs assert."""
    from niidmix import logger as nl
    logger, nodes, _ = _fake_logger(monkeypatch, tmp_path, **{
        "log-global-model-accuracy": True, "skip-training": True, "skip-testing": True,
        "skip-validation": True, "skip-full-training": True})
    averaged = []
    center = Net()
    monkeypatch.setattr(nl, "average", lambda models, weights=None: averaged.append(list(models)) or center)
    ev = _StubEvaluator()
    out = nl.state_events(ev, logger, nodes, {"step": 5})
    assert averaged == [[nodes[0]["model"], nodes[1]["model"]]]
    assert ev.calls == [("full-train", ["center"]), ("test", ["center"]), ("valid", ["center"])]
    assert [p for p, _ in out] == [logger.global_events] * 3
    assert [e["data"] for _, e in out] == ["train", "test", "valid"]
    assert all(list(e) == GLOBAL_KEYS and e["epoch"] == 2 and e["step"] == 5 for _, e in out)
    assert [(e["accuracy"], e["loss"]) for _, e in out] == [(0.3 + 0.05, 10 * 0.3), (0.1 + 0.05, 10 * 0.1),
                                                          (0.2 + 0.05, 10 * 0.2)]
    nodes[1]["epoch"] = 3
    with pytest.raises(AssertionError, match="Inconsistent epochs"):
        nl.state_events(ev, logger, nodes, {"step": 6})


def test_device_state_writes_the_files(monkeypatch, tmp_path):
    """The installed Logger.state appends one JSON line per event to the reference's files and
    makes no other file."""
    from niidmix import evaluate, logger as nl
    logger, nodes, params = _fake_logger(monkeypatch, tmp_path, **{"log-global-model-accuracy": True})
    assert "simulate.logger.Logger.state" in nl.install_hooks(params)
    ev = _StubEvaluator()
    monkeypatch.setattr(evaluate, "default", lambda p: ev)
    monkeypatch.setattr(nl, "average", lambda models, weights=None: Net())
    logger.state([], {"step": 3})
    assert ev.calls == []
    logger.state(nodes, {"step": 3})
    assert sorted(os.listdir(tmp_path)) == ["events"]
    assert sorted(os.listdir(tmp_path / "events")) == ["1.jsonlines", "3.jsonlines", "global.jsonlines"]
    for r in (1, 3):
        lines = [json.loads(ln) for ln in open(tmp_path / "events" / f"{r}.jsonlines")]
        assert [e["data"] for e in lines] == ["train", "test", "valid", "full-train"]
        assert all(e["rank"] == r for e in lines)
    lines = [json.loads(ln) for ln in open(tmp_path / "events" / "global.jsonlines")]
    assert [e["data"] for e in lines] == ["train", "test", "valid"]


def test_install_hooks_with_and_without_the_flag(monkeypatch, tmp_path):
    from niidmix import logger as nl
    logger, _, _ = _fake_logger(monkeypatch, tmp_path)
    cls = type(logger)
    ref_state = cls.state
    monkeypatch.delitem(sys.modules, "setup.model", raising=False)
    off = nl.install_hooks({"logger": {}, "algorithm": {}})
    assert off == ["simulate.logger.Logger.log_consensus_distance"] and cls.state is ref_state
    assert nl.install_hooks({"logger": {}}) == off and cls.state is ref_state
    on = nl.install_hooks({"logger": {}, "algorithm": {"device-evaluation": True}})
    assert on == off + ["simulate.logger.Logger.state"] and cls.state is nl.device_state
    assert nl.install_hooks({"logger": {}, "algorithm": {"device-evaluation": True}}) == on
    monkeypatch.delitem(sys.modules, "simulate.logger")
    assert nl.install_hooks({"logger": {}, "algorithm": {"device-evaluation": True}}) == []


def _params(**alg):
    a = {"learning-rate": 0.1, "learning-momentum": 0.0, "batch-size": 16, "initial-averaging": False,
         "clique-gradient": False, "unbiased-gradient": False, "device-evaluation": True}
    a.update(alg)
    return {"meta": {"log": "WARNING"}, "topology": {"name": "ring"}, "algorithm": a, "logger": {}}


def _nodes(params, models):
    from niidmix import d_sgd
    return [{"rank": r, "epoch": 0, "train-set": [(torch.zeros(6), 0)] * 4, "model": mdl,
             "optimizer": d_sgd.optimizer(mdl, params)} for r, mdl in enumerate(models)]


def test_eval_refusals_name_the_flag():
    from niidmix import d_sgd, evaluate
    p = _params()
    with pytest.raises(ValueError, match="device-evaluation"):
        d_sgd.init(_nodes(p, [Net(), Net3()]), {"edges": {}}, p)
    with pytest.raises(ValueError, match="device-evaluation"):
        d_sgd.init(_nodes(p, [Net(), Net(k=7)]), {"edges": {}}, p)
    with pytest.raises(ValueError, match="device-evaluation"):
        d_sgd.init(_nodes(p, [Net(c=1025)]), {"edges": {}}, p)
    with pytest.raises(ValueError, match="device-evaluation"):
        evaluate.check_eligible([], p)
    state, _, _ = d_sgd.init(_nodes(p, [Net(), Net()]), {"edges": {}}, p)          # eligible
    assert state["step"] == 0
    p = _params(**{"device-evaluation": False})
    d_sgd.init(_nodes(p, [Net(), Net3()]), {"edges": {}}, p)                       # off: not looked at
    ev = evaluate.DeviceEvaluator(_params(), device="cpu")
    with pytest.raises(ValueError, match="device-evaluation"):
        ev._set("nonsense")
    saved = sys.modules.pop("setup.dataset", None)
    try:
        with pytest.raises(ValueError, match="device-evaluation.*register"):
            ev._set("test")                                # neither registered nor loadable
    finally:
        if saved is not None:
            sys.modules["setup.dataset"] = saved


def test_cli_flag_is_a_store_const(tmp_path, monkeypatch):
    from niidmix import d_sgd
    for argv, want in (([], None), (["--device-evaluation"], True),
                       (["--device-evaluation", "--device-training"], True)):
        run = tmp_path / str(len(argv))
        run.mkdir()
        (run / "params.json").write_text(json.dumps({"topology": {"name": "ring"}}))
        monkeypatch.setattr(d_sgd, "load_topology", lambda rundir: {"edges": {}})
        d_sgd.main(["--rundir", str(run)] + argv)
        alg = json.loads((run / "params.json").read_text())["algorithm"]
        assert alg.get("device-evaluation") is want
        assert alg.get("device-training") is (True if "--device-training" in argv else None)
