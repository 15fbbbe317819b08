"""Accuracy and loss of linear and GN-LeNet models on the device (`--device-evaluation`).

The reference's logger evaluates every logged node with CPU DataLoader loops: its own train-set
in Logger.log_train_accuracy (tools/simulate/logger.py:205-249), and the shared validation, test
and full train sets in worker processes it reaches over ssh (logger.py:166-185,
tools/simulate/run_logger.py).  For the reference's linear model (setup/model/linear.py: one
nn.Linear(K, C), log_softmax) DeviceEvaluator computes the same numbers in one kernel call per
set for all nodes at once (niidmix::linear_eval_rows):

    parameters   a live DeviceTrainer's device slab, read in place (--device-training and
                 --device-training-gn-lenet; no upload),
                 else the models' parameters stacked and uploaded once per call
    sets         materialised once as [M, K] fp32 + int32 labels in HBM (register_sets); the
                 nodes' own train-sets are the trainer's when one is live
    accuracy(models_or_nodes, set_name)   run_logger.model_accuracy: (correct / M, loss_sum / M)
    train_accuracy(nodes)                 Logger.log_train_accuracy: chunks of 1000 samples,
                                          (total correct / total samples, mean of the chunks' mean
                                          losses)

The reference's other model, GN-LeNet (setup/model/gn_lenet.py: three 5 x 5 convolutions with
GroupNorm(2), max-pooling and ReLU, then one Linear), goes through niidmix::gnlenet_eval_rows the
same way.  Its parameters are read in place from a fresh single-stripe resident round's output slab
(niidmix.slab.ResidentRound, on its mixing stream), else stacked and uploaded; the job list of a
call is cut (niidmix.train.cut_rows) so that the kernel's scratch stays within a fraction of the
free HBM (a job's results do not depend on the cut).

What depends on the model family -- shapes, limits, the sample check, the evaluation op and its
scratch, the forward probe -- is niidmix.family's; DeviceEvaluator calls through the family of the
models it is given.

Not bit-identical to the CPU loops (another summation order; tests/test_gpu_eval.py and
tests/test_gpu_eval_gnlenet.py state the bounds), so the path is opt-in.  A model that is neither
log_softmax(Linear) nor GN-LeNet is refused with a ValueError naming the flag: there is no silent
CPU fallback.
"""
import sys

import torch

from . import family, train
from .model import flatten

FLAG = "--device-evaluation"
CHUNK = 1000          # Logger.log_train_accuracy's DataLoader batch size (logger.py:217)
SET_NAMES = ("valid", "test", "full-train")
SCRATCH_FRACTION = 0.8   # of the free HBM, for one call's scratch (DeviceTrainer._check_fit's rule)


def enabled(params):
    return bool(params.get("algorithm", {}).get("device-evaluation"))


def chunk_jobs(offsets, chunk=CHUNK):
    """The (node, chunk) jobs of train_accuracy: offsets [n + 1] are the nodes' sample ranges in
    one concatenated array.  Returns (node index, segment start, segment length) lists: each node's
    range cut into consecutive chunks of `chunk` samples, the last one short."""
    node, start, length = [], [], []
    for i in range(len(offsets) - 1):
        for s in range(offsets[i], offsets[i + 1], chunk):
            node.append(i)
            start.append(s)
            length.append(min(chunk, offsets[i + 1] - s))
    return node, start, length


def fold_chunks(n_nodes, node, length, loss_sum, correct):
    """[(accuracy, loss)] per node from its chunks' summed losses and correct counts: accuracy is
    total correct over total samples, loss the mean over chunks of each chunk's mean loss
    (logger.py:223-228, :243-245); (0.0, 0.0) for a node without samples."""
    tot = [[0, 0, 0.0, 0] for _ in range(n_nodes)]      # correct, samples, sum of means, chunks
    for i, ln, ls, c in zip(node, length, loss_sum, correct):
        t = tot[i]
        t[0] += int(c)
        t[1] += int(ln)
        t[2] += float(ls) / ln
        t[3] += 1
    return [(t[0] / t[1], t[2] / t[3]) if t[1] else (0.0, 0.0) for t in tot]


def check_eligible(nodes, params):
    """The refusals that need no GPU (d_sgd.init calls this): raises ValueError naming the flag.
    Returns (K, C) for linear models and (Cin, C, F) for GN-LeNet."""
    if not nodes:
        raise ValueError(f"{FLAG}: no nodes")
    return _shape([nd["model"] for nd in nodes])[1]


def _shape(models):
    """(family, shape) of a model list that is all-linear (family.LINEAR, (K, C)) or all-GN-LeNet
    (family.GN_LENET, (Cin, C, F)), of one shape."""
    fam, shape = family.family_of(models[0]) or (None, None)
    for i, mdl in enumerate(models):
        if fam is None or fam.shape(mdl) != shape:
            raise ValueError(f"{FLAG} needs models whose parameters are exactly a [C, K] weight and "
                             f"a [C] bias, or exactly GN-LeNet's 14 tensors, the same on every model "
                             f"(model {i} differs)")
    fam.limits(shape, FLAG)
    return fam, shape


class _Set:
    """A sample set in HBM: data [M, K] fp32 (the samples flattened), labels [M] int32, the shape
    of one sample as the model takes it ((Cin, H, W) for images), and its first samples in that
    shape (for the forward probe)."""

    def __init__(self, data, labels, lo, hi, probe):
        self.data, self.labels, self.lo, self.hi, self.probe = data, labels, lo, hi, probe
        self.m = int(labels.shape[0])
        self.shape = tuple(probe[0].shape[1:]) if probe is not None else None


def _materialise(source, device, what):
    """Any dataset or DataLoader of (x, y) -> _Set on `device`."""
    loader = source if isinstance(source, torch.utils.data.DataLoader) else \
        torch.utils.data.DataLoader(source, batch_size=CHUNK)
    xs, ys, probe = [], [], None
    for x, y in loader:
        x, y = torch.as_tensor(x), torch.as_tensor(y)
        if probe is None:
            probe = (x[:family.PROBE_SAMPLES].clone(), y[:family.PROBE_SAMPLES].to(torch.int64).clone())
        xs.append(x.reshape(x.shape[0], -1).to(torch.float32))
        ys.append(y.reshape(-1).to(torch.int64))
    dev = torch.device(device)
    if not xs:
        return _Set(torch.empty((0, 1), dtype=torch.float32, device=dev),
                    torch.empty(0, dtype=torch.int32, device=dev), 0, -1, None)
    if len({x.shape[1] for x in xs}) != 1:
        raise ValueError(f"{FLAG}: the samples of {what} do not flatten to one size")
    x, y = torch.cat(xs).contiguous(), torch.cat(ys)
    if x.shape[0] >= 2 ** 31:
        raise ValueError(f"{FLAG}: {x.shape[0]} samples in {what} exceed int32 indices")
    need = x.numel() * 4 + y.numel() * 4
    free, _ = torch.cuda.mem_get_info(dev)
    if need > 0.8 * free:              # DeviceTrainer._check_fit's rule
        raise RuntimeError(f"{FLAG}: {need / 2**30:.1f} GiB of samples ({what}) do not fit in "
                           f"{free / 2**30:.1f} GiB of free HBM")
    return _Set(x.to(dev), y.to(torch.int32).to(dev), int(y.min()), int(y.max()), probe)


class DeviceEvaluator:
    def __init__(self, params, device=None):
        self.params = params
        self.device = torch.device(device) if device is not None else None
        self.sets = {}
        self.last_source = None          # "trainer" / "resident" (device slab read in place) or "stacked"
        self.scratch_budget = None       # bytes of scratch per GN-LeNet call (None: SCRATCH_FRACTION
        self.last_calls = 0              # of the free HBM), and the calls the last job list took
        self._probed = set()             # (model class, kind, sizes) whose forward was probed
        self._train = None               # (train-sets, _Set, offsets) of the last node list

    def _dev(self):
        if self.device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        return self.device

    # -------------------------------------------------------------------------------------------
    def register_sets(self, valid=None, test=None, full_train=None):
        """Datasets or DataLoaders of (x, y) for accuracy(.., "valid" / "test" / "full-train"),
        copied to the device once."""
        for name, src in (("valid", valid), ("test", test), ("full-train", full_train)):
            if src is not None:
                self.sets[name] = _materialise(src, self._dev(), f"the {name} set")
        return self

    def _set(self, name):
        name = name.replace("_", "-")
        if name not in SET_NAMES:
            raise ValueError(f"{FLAG}: unknown set {name!r} (one of {', '.join(SET_NAMES)})")
        if name not in self.sets:
            ds = sys.modules.get("setup.dataset")
            fn = getattr(ds, {"valid": "valid", "test": "test", "full-train": "train"}[name], None)
            if not callable(fn):
                raise ValueError(f"{FLAG}: no {name} set: register it "
                                 "(niidmix.evaluate.register_sets) before the first logged step")
            self.sets[name] = _materialise(fn(self.params), self._dev(), f"the {name} set")
        return self.sets[name]

    def _check(self, st, spec, what):
        """Refuses a set the models do not take; returns the kernel's size arguments: (K, C) for
        linear models, (Cin, H, W, C) for GN-LeNet."""
        fam, shape = spec
        c = shape[1]
        if st.m and (st.lo < 0 or st.hi >= c):
            raise ValueError(f"{FLAG}: {what} has a label outside [0, {c})")
        return fam.sizes(st.shape, shape, FLAG, what)

    def _probe(self, model, st, spec, sizes):
        key = (type(model), spec[0].kind) + tuple(sizes)
        if key in self._probed or st.probe is None:
            return
        try:
            spec[0].probe_eval(model, st.probe[0], st.probe[1], self.params, self._dev(), sizes, FLAG)
        except ValueError:
            raise
        except Exception as e:         # a forward that does not take these samples at all
            raise ValueError(f"{FLAG}: the model's forward failed on the set's samples "
                             f"({type(e).__name__}: {e}); only log_softmax(Linear) and GN-LeNet are "
                             "evaluated")
        self._probed.add(key)

    # -------------------------------------------------------------------------------------------
    def _theta(self, models):
        """(theta slab [*, P] on the device, row of each model, (family, shape), the stream the slab
        must be read on or None for the current one)."""
        from . import d_sgd
        spec = _shape(models)
        p = spec[0].P(spec[1])
        hit = d_sgd.device_trainer(models)           # a live trainer's slab, of either kind
        if hit is not None and hit[0].p == p:
            tr, rows = hit
            if self.device is None or tr.device == self.device:
                cur = tr.current()
                if cur is not None:
                    self.device = tr.device
                    self.last_source = "trainer"
                    return cur, rows, spec, None
        if spec[0].reads_resident:
            from . import logger as nl
            hit = nl._fresh_resident(models)
            if hit is not None and len(hit[0].parts) == 1 and hit[0].p == p:
                pt = hit[0].parts[0]
                if self.device is None or pt["dev"] == self.device:
                    self.device = pt["dev"]
                    self.last_source = "resident"
                    return pt["outs"][0], hit[1], spec, pt["s_mix"]
        d_sgd.synchronize()              # the models must hold the last round's rows
        theta = torch.zeros((len(models), train.padded_ld(p)), dtype=torch.float32,
                            device=self._dev())[:, :p]
        theta.copy_(flatten(models, "cpu"))
        self.last_source = "stacked"
        return theta, list(range(len(models))), spec, None

    def _cut(self, fam, n, max_len, sizes, dev):
        """Jobs per call of the family's kernel: all of them for a family whose calls are not cut,
        else as many as keep the call's scratch within the budget (train.cut_rows)."""
        if not fam.cut:
            return n
        budget = self.scratch_budget
        if budget is None:
            budget = SCRATCH_FRACTION * torch.cuda.mem_get_info(dev)[0]
        need = lambda k: fam.eval_scratch_bytes(k, max_len, sizes)  # noqa: E731
        k = train.cut_rows(n, need, budget)
        if k is None:
            raise RuntimeError(f"{FLAG}: {need(1) / 2**30:.2f} GiB of scratch for one job of "
                               f"{max_len} samples exceed the budget of {budget / 2**30:.2f} GiB")
        return k

    def _run(self, theta, st, rows, start, length, spec, sizes, stream=None):
        dev, fam = theta.device, spec[0]
        with torch.cuda.device(dev), torch.cuda.stream(stream or torch.cuda.current_stream(dev)):
            n = len(rows)
            idx = torch.tensor([rows, start, length], dtype=torch.int32).to(dev)
            loss = torch.empty(n, dtype=torch.float64, device=dev)
            correct = torch.empty(n, dtype=torch.int32, device=dev)
            cut = self._cut(fam, n, max(length), sizes, dev)
            starts = range(0, n, cut)
            if fam.cut:                  # as it was: a list that is never cut leaves the count alone
                self.last_calls = len(starts)
            for a in starts:
                b = min(n, a + cut)
                fam.eval_rows(theta, st.data, st.labels, idx[0, a:b], idx[1, a:b], idx[2, a:b],
                              max(length[a:b]), loss[a:b], correct[a:b], sizes)
            # read back on the same stream: a copy on another one would not wait for the kernel
            return loss.cpu().tolist(), correct.cpu().tolist()

    @staticmethod
    def _models(items):
        return [it["model"] if isinstance(it, dict) else it for it in items]

    def accuracy(self, models_or_nodes, set_name):
        """[(accuracy, loss)] of every model on a registered set: correct / M and loss_sum / M;
        (0.0, 0.0) for an empty set."""
        models = self._models(models_or_nodes)
        if not models:
            return []
        theta, rows, spec, stream = self._theta(models)
        st = self._set(set_name)
        if st.m == 0:
            return [(0.0, 0.0) for _ in models]
        sizes = self._check(st, spec, f"the {set_name} set")
        self._probe(models[0], st, spec, sizes)
        loss, correct = self._run(theta, st, rows, [0] * len(rows), [st.m] * len(rows), spec, sizes,
                                  stream)
        return [(cr / st.m, ls / st.m) for ls, cr in zip(loss, correct)]

    def _train_sets(self, nodes, theta_dev):
        """The nodes' own train-sets in one array: a live trainer's, else materialised (kept while
        the same train-set objects are asked for)."""
        from . import d_sgd
        hit = d_sgd.device_trainer([nd["model"] for nd in nodes])
        if hit is not None and hit[0].device == theta_dev:
            tr, rows = hit
            ts = nodes[0]["train-set"]
            probe = None
            if len(ts):
                items = [ts[j] for j in range(min(family.PROBE_SAMPLES, len(ts)))]
                probe = (torch.stack([torch.as_tensor(s[0]) for s in items]),
                         torch.as_tensor([int(s[1]) for s in items], dtype=torch.int64))
            st = _Set(tr.data, tr.labels, 0, tr.c - 1, probe)
            return st, [(tr.offsets[r], tr.offsets[r + 1]) for r in rows]
        sets = [nd["train-set"] for nd in nodes]
        if self._train is None or len(self._train[0]) != len(sets) or \
                any(a is not b for a, b in zip(self._train[0], sets)):
            offsets = [0]
            for ts in sets:
                offsets.append(offsets[-1] + len(ts))
            st = _materialise(torch.utils.data.ConcatDataset(sets), theta_dev, "the nodes' train-sets")
            self._train = (sets, st, offsets)
        _, st, offsets = self._train
        return st, [(offsets[i], offsets[i + 1]) for i in range(len(sets))]

    def train_accuracy(self, nodes):
        """[(accuracy, loss)] of every node on its own train-set, as Logger.log_train_accuracy:
        one job per (node, chunk of 1000 samples), all nodes in one call."""
        nodes = list(nodes)
        if not nodes:
            return []
        theta, rows, spec, stream = self._theta([nd["model"] for nd in nodes])
        st, ranges = self._train_sets(nodes, theta.device)
        sizes = self._check(st, spec, "the nodes' train-sets") if st.m else None
        node, start, length = [], [], []
        for i, (a, b) in enumerate(ranges):
            nd, s, ln = chunk_jobs([a, b])
            node += [i] * len(nd)
            start += s
            length += ln
        if not node:
            return [(0.0, 0.0) for _ in nodes]
        self._probe(nodes[0]["model"], st, spec, sizes)
        loss, correct = self._run(theta, st, [rows[i] for i in node], start, length, spec, sizes,
                                  stream)
        return fold_chunks(len(nodes), node, length, loss, correct)


# the evaluator the logger hook uses (niidmix.logger.device_state), one per params object
_default = None


def default(params):
    global _default
    if _default is None or _default.params is not params:
        sets = _default.sets if _default is not None else {}
        _default = DeviceEvaluator(params)
        _default.sets = sets             # sets registered before the run's params were known
    return _default


def register_sets(valid=None, test=None, full_train=None, params=None):
    """Register the shared sets with the hook's evaluator (call it before the first logged step)."""
    global _default
    if _default is None:
        _default = DeviceEvaluator(params if params is not None else {})
    elif params is not None:
        default(params)
    return _default.register_sets(valid=valid, test=test, full_train=full_train)
