"""A training step without torch in its tail: StackTrainer runs

    the model's fused stack (one forward launch)  ->  ops.head_loss (dropout, head, cross entropy and every gradient)
    ->  the stack's backward (one launch and a reduction)  ->  ops.adam_step (every parameter, one launch)

on a device step counter that both the dropout mask and Adam's bias corrections read, so the whole step of a fixed batch
can be captured once (torch.cuda.graph) and replayed: the regime of the notebook, one 188-graph batch for 60 steps.

NodeTrainer is the same for node classification (sgrace.GAT_PYNQ): the model's two layers through their own autograd,
ops.NodeLoss (the tail over the selected rows, the count of which never leaves the device) and ops.adam_step.

BestTracker (trainer.track_best()) is the loop's model selection on the device: one ops.keep_best per epoch keeps the
weights of the epoch that evaluated best and logs every epoch's sums, so a run is read back once.
"""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from . import ops


class _Trainer:
    """What the two trainers share: the optimiser state (exp_avg, exp_avg_sq per parameter, the device step counter `t`),
    its copies, the Adam call that ends a step and the capture of a step.  A trainer adds step(*batch)."""

    def __init__(self, model, lr, betas, eps, weight_decay, p_drop, seed):
        self.model = model
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.p_drop, self.seed = float(p_drop), int(seed)
        self.params = [p for p in model.parameters() if p.requires_grad]
        dev = self.params[0].device
        self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.t = torch.zeros(1, dtype=torch.int64, device=dev)
        self.last_grads = None        # the gradients handed to the last ops.adam_step, in self.params' order

    def _adam(self, grads):
        """One ops.adam_step over self.params with `grads` (None: that parameter is skipped), kept as last_grads."""
        grads = [None if g is None else g.contiguous() for g in grads]
        ops.adam_step(self.params, grads, self.exp_avg, self.exp_avg_sq, self.t, lr=self.lr, betas=self.betas, eps=self.eps,
                      weight_decay=self.weight_decay)
        self.last_grads = grads

    def state(self):
        """Copies of everything a step changes: the parameters, both moments, the counter."""
        return [t.detach().clone() for t in (*self.params, *self.exp_avg, *self.exp_avg_sq, self.t)]

    def load_state(self, state):
        with torch.no_grad():
            for dst, src in zip((*self.params, *self.exp_avg, *self.exp_avg_sq, self.t), state):
                dst.copy_(src)

    def track_best(self, epochs=None):
        """A BestTracker over this trainer's parameters: the best epoch's weights kept on the device, a run read back once.
        epochs: the rows of its log (None: no log)."""
        return BestTracker(self, epochs)

    def _capture(self, batch, warmup, probe=None, counters=(), run=None, guard_workspace=False):
        """Record self.step(*batch) (or run(), where a step has more in front of it) with torch.cuda.graph (one stream, no parallel branches) and return a callable that
        replays it and returns the loss tensor the replay fills.  The warm-up steps it needs first (they build what a step
        caches: the CSRs, the plans, the workspaces) run on a side stream on a copy of the state, which is put back before
        the capture: the trainer is where it was, and n replays equal n eager steps.  probe: run on the side stream after
        the warm-up steps; what it returns is raised once the state is back.  counters: the names of host-side counts that
        the recorded step (which computes nothing until it is replayed) must leave as the warm-up left them.

        guard_workspace: ops._workspace keeps one grow-only scratch tensor per stream, and a recording holds the address
        it saw.  The recording is then made ON the warm-up's stream, so that every call it runs has already asked that
        stream's workspace for its size; the tensor's address is compared before and after the capture, and RuntimeError
        is raised -- no recording is returned -- if a call inside the recording replaced it (an earlier launch of the
        same recording would hold the old address).  The recording keeps a reference to the tensor (replay.workspace), so
        that its memory outlives a later growth of that stream's workspace.  A host-side check; nothing synchronises."""
        if run is None:
            run = lambda: self.step(*batch)
        saved = self.state()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                run()
            failure = probe() if probe is not None else None
        torch.cuda.current_stream().wait_stream(side)
        self.load_state(saved)
        for p in self.params:
            p.grad = None
        if failure is not None:
            raise failure
        kept = [(name, getattr(self, name)) for name in counters]
        graph = torch.cuda.CUDAGraph()
        workspace = moved = None
        if guard_workspace:
            key = (self.t.device.index, side.cuda_stream)
            address = lambda: getattr(ops._workspaces.get(key), "data_ptr", lambda: None)()
            workspace, before = ops._workspaces.get(key), address()
            side.wait_stream(torch.cuda.current_stream())          # (the state was put back on the current stream)
            with torch.cuda.graph(graph, stream=side):
                loss = run()
            moved = address() != before
        else:
            with torch.cuda.graph(graph):
                loss = run()
        for name, value in kept:
            setattr(self, name, value)
        if moved:
            raise RuntimeError("the recorded step replaced its stream's workspace (ops._workspace) in the middle of the "
                               "recording: a call in it asked for more scratch than the warm-up steps did, and an earlier "
                               "launch of the recording holds the old address; nothing was recorded")

        def replay():
            graph.replay()
            return loss

        replay.graph, replay.workspace = graph, workspace
        return replay

    @contextlib.contextmanager
    def _eval_mode(self):
        """Around one batch of an evaluation: the model in eval mode with gradients off; its mode is put back."""
        model = self.model
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                yield model
        finally:
            model.train(was_training)

    @staticmethod
    def _eval_pass(sums, walk, one, result, **attrs):
        """What the two capture_eval_loader return: the callable of a whole pass over the loader behind `walk` (the trainer's
        _capture_padded made it) -- the EvalSums `sums` zeroed (one launch), every padded batch replayed, every batch that
        arrives unpadded run through one(batch) into the same sums -> `result`.  It carries sums and attrs as attributes."""
        def run_pass():
            sums.zero_()
            walk(lambda _: None, one)
            return result

        run_pass.sums = sums
        for name, value in attrs.items():
            setattr(run_pass, name, value)
        return run_pass


class StackTrainer(_Trainer):
    """Adam on the kernels for GCN_PYNQ(train_stack=True) / GAT_POOL_PYNQ(train_stack=True) (fake quantisation included).

        trainer = StackTrainer(model, lr=0.01)
        loss = trainer.step(x, edge_index, batch, y)          # a device tensor [1]; nothing synchronises
        replay = trainer.capture(x, edge_index, batch, y)     # the step of this batch, recorded once
        loss = replay()
        epoch = trainer.capture_loader(loader)                # a GraphLoader(pad=True): one recorded step for every batch
        losses = epoch()                                      # one shuffled epoch, a loss tensor per batch
        totals, loss_sum = trainer.evaluate(x, edge_index, batch, y)      # device int64 [graphs, hits], device float64 [1]
        test = trainer.capture_eval_loader(test_loader)       # a GraphLoader(pad=True): one recorded evaluation for every batch
        totals, loss_sum = test()                             # one pass over the set, summed on the device

    The trainer owns the optimiser state (exp_avg, exp_avg_sq per parameter, the device step counter `t`); its dropout
    stream is ops.head_loss's counter-based mask of (seed, t), not torch's generator.  step() is a training step whatever
    model.training says: dropout p_drop is applied on every route that runs the one-call tail.  Where the model's fused
    route declines a batch (it does not fit the plan, has dead rows) the step runs the model's layers one by one
    (model.layers_pooled) with ops.HeadLoss behind them -- the same tail, p_drop and mask stream.  Only where `batch` is
    not sorted, so that the model pools inside its own forward, the step is the model's forward with torch's tail: its
    dropout is the model's (p = 0.5 from torch's generator, in training mode only), p_drop and seed do not apply.  Every
    route updates through the same ops.adam_step on the same state."""

    def __init__(self, model, lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, p_drop=0.5, seed=12345):
        if not hasattr(model, "train_pooled") or not hasattr(model, "layers_pooled") or not hasattr(model, "lin"):
            raise TypeError("StackTrainer takes a GCN_PYNQ or a GAT_POOL_PYNQ")
        super().__init__(model, lr, betas, eps, weight_decay, p_drop, seed)
        self.fused_steps = 0          # steps that took the fused route (host-side count; a replay counts nothing)

    def _forward(self, x, edge_index, batch):
        from .molecule_gcn import GCN_PYNQ
        if isinstance(self.model, GCN_PYNQ):
            return self.model(1, x, edge_index, batch)
        return self.model(x, edge_index, batch)

    def step(self, x, edge_index, batch, y, n_real=None):
        """One training step -> the loss, a device tensor [1].  n_real: the real graph count of a padded batch
        (Batch.num_real_graphs); the loss head then runs on the first n_real pooled rows and labels, and the filler graphs
        behind them receive a zero gradient.  A padded batch runs the fused route or not at all: where the model declines
        it, RuntimeError names the reason before anything is changed (the layer-by-layer routes were written for CSRs
        without spare capacity; pyg_lite.GraphLoader(pad=True) delivers the batches it knows to be declined unpadded)."""
        model = self.model
        for p in self.params:
            p.grad = None
        head = {id(model.lin.weight): None, id(model.lin.bias): None}
        pooled = model.train_pooled(x, edge_index, batch)
        if n_real is not None and n_real != y.shape[0]:
            y = y[:n_real]
        else:
            n_real = None
        if pooled is not None:
            rows = pooled if n_real is None else pooled.detach()[:n_real]
            loss, grad_pooled, grad_w, grad_b = ops.head_loss(rows, model.lin.weight, model.lin.bias, y, p=self.p_drop,
                                                              seed=self.seed, step=0, step_dev=self.t)
            if n_real is not None:
                grad_pooled = F.pad(grad_pooled, (0, 0, 0, pooled.shape[0] - n_real))
            pooled.backward(grad_pooled)
            head = {id(model.lin.weight): grad_w, id(model.lin.bias): grad_b}
            self.fused_steps += 1
        else:
            if self._is_padded(batch):
                raise RuntimeError(f"StackTrainer.step: the fused route declined a padded batch: {self._declined(batch)}")
            pooled = model.layers_pooled(x, edge_index, batch)
            if pooled is not None:
                # the layers one by one with their own autograd; the tail is still the one call, on the same mask stream
                rows = pooled if n_real is None else pooled[:n_real].contiguous()
                loss = ops.HeadLoss.apply(rows, model.lin.weight, model.lin.bias, y, self.p_drop, self.seed, 0, self.t)
            else:
                logits = self._forward(x, edge_index, batch)
                loss = F.cross_entropy(logits if n_real is None else logits[:n_real], y)
            loss.backward()
            loss = loss.detach().reshape(1)
        self._adam([head.get(id(p)) if head.get(id(p)) is not None else p.grad for p in self.params])
        return loss

    def capture(self, x, edge_index, batch, y, warmup=2):
        """Record one step on this batch with torch.cuda.graph (one stream, no parallel branches) and return a callable
        that replays it and returns the loss tensor the replay fills.  The warm-up steps it needs first (they build what
        a step caches: the CSRs, the plan, the workspace) run on a copy of the state, which is put back before the
        capture: the trainer is where it was, and n replays equal n eager steps."""
        return self._capture((x, edge_index, batch, y), warmup, counters=("fused_steps",))

    @staticmethod
    def _block_facts(batch):
        """The block facts a GraphLoader recorded for the batch vector `batch`, or None (nothing is built or read back)."""
        ptr = ops.recorded(batch, ("graph_ptr",))
        return None if ptr is None else ops.recorded(ptr, ("block_facts",))

    def _is_padded(self, batch):
        return bool((self._block_facts(batch) or {}).get("padded"))

    def _declined(self, batch, training=True):
        """Why model.train_pooled (training=False: model.eval_pooled) declined the padded batch of batch vector `batch`, as
        far as it can be told from outside."""
        model = self.model
        if training and not getattr(model, "train_stack", False):
            return "the model was not built with train_stack=True"
        if not model._stack_enabled():
            return "the register layer_count is under 2 (or the kernels are off): the layers run one by one"
        if training and not torch.is_grad_enabled():
            return "gradients are disabled"
        facts = self._block_facts(batch)
        quantised = ("; with the quantiser on (config.fake_quantization / hardware_quantize) also: config.float_type is "
                     "float32, the quantiser constants are set (sgrace.init_SGRACE after the config), no row is dead under "
                     "the QUANTISED adjacency, and not both config.hardware_quantize and a hidden width over 128 (the int8 form)")
        if not training:
            return ("a condition of the model's fused eval route fails on the padded batch (its class docstring lists them): "
                    "no row of the adjacency may be dead" + quantised)
        return (f"a condition of the model's fused training route fails on the padded batch (its class docstring lists "
                f"them); the largest graph of the set has {facts['max_graph'] if facts else '?'} rows, which must be within "
                f"the backward plan's row budget, and no row of the adjacency may be dead" + quantised)

    def capture_loader(self, loader, warmup=2):
        """One recorded step for every padded batch of `loader` (a pyg_lite.GraphLoader(pad=True)) -> a callable that runs
        one epoch and returns its losses, one device tensor [1] per batch, in the loader's order.

        The recorded step is the padded collation (ops.collate_graphs(pad=) into one capacity-sized ops.Collated, with the
        cached plans' table launches behind it), the fused forward, ops.head_loss on the real graphs, the fused backward and
        ops.adam_step -- one stream, no parallel branches, as capture().  An epoch draws its batches as iterating the
        loader would (one draw from its generator), uploads the graph ids and offsets of all its padded batches once, and
        per padded batch copies that batch's row into the static index buffer (device to device) and replays.  A batch
        that arrives unpadded -- a short last batch, a batch over pad_rows, a batch with a dead-row graph (a host fact of
        the prepared set; the fused GAT route declines it) -- runs through step() unpadded in its place, so an epoch
        takes exactly the steps of `for b in loader: step(b.x, b.edge_index, b.batch, b.y, b.num_real_graphs)`.
        The warm-up steps run on a padded batch of the set's smallest graphs without a dead row, on a copy of the state.
        If the model's fused route declines that batch, RuntimeError names the reason: a padded batch never falls back.
        A loader with quant= and pad_quant=True serves GAT_POOL_PYNQ(train_stack=True) with the quantiser on (attention
        and GCN layers, config.fake_quantization with and without config.hardware_quantize, hidden <= 128): the padded
        batches carry the quantised adjacencies, a batch with a graph dead under the quantised mask arrives unpadded too,
        and the recording is made on the warm-up's stream under _capture's workspace guard (RuntimeError, and no
        recording, if a call in it replaced the stream's workspace)."""
        def accepts(b):
            with torch.enable_grad():                  # (before any state is touched: step() raises on a declined padded batch)
                if self.model.train_pooled(b.x, b.edge_index, b.batch) is None:
                    raise RuntimeError(f"StackTrainer.capture_loader: the fused route declined the padded batch: {self._declined(b.batch)}")

        replay, c, walk = self._capture_padded(loader, warmup, "capture_loader", accepts,
                                               lambda b: self.step(b.x, b.edge_index, b.batch, b.y, b.num_real_graphs),
                                               counters=("fused_steps",))

        def epoch():
            losses = []
            walk(lambda loss: losses.append(loss.clone()),
                 lambda e: losses.append(self.step(e.x, e.edge_index, e.batch, e.y, e.num_real_graphs)))
            return losses

        epoch.graph, epoch.collated = replay.graph, c
        return epoch

    def _capture_padded(self, loader, warmup, name, accepts, run_batch, counters=()):
        """What capture_loader and capture_eval_loader share: ONE recording of run_batch(b) on the padded batch b of
        `loader` (a pyg_lite.GraphLoader(pad=True); anything else: ValueError) behind its collation -> (replay, the
        capacity-sized ops.Collated the recording reads, walk).  The recording runs on a padded batch of the set's
        smallest graphs without a dead row; accepts(b) raises first where the model would decline it.  walk(replayed,
        eager) takes one pass over the loader as iterating it would (one draw from its generator): the graph ids and
        offsets of all its padded batches are uploaded once (pinned, non-blocking), and per padded batch that batch's row
        is copied into the static index buffer (device to device), the recording replayed and replayed(what run_batch
        returned) called; a batch that arrives unpadded is collated unpadded and handed to eager(batch) in its place."""
        from . import pyg_lite
        if not getattr(loader, "pad", False):
            raise ValueError(f"{name} takes a GraphLoader(pad=True)")
        gs, cap, B = loader.graphs, loader.capacity, loader.capacity.batch_size
        quant = bool(getattr(loader, "pad_quant", False))          # the loader's mode: its padded batches carry the quantised adjacencies
        rows = gs.counts[0]
        dead = loader.has_dead() if loader.extras is not None else np.zeros(len(gs), dtype=bool)
        first = [int(g) for g in np.argsort(rows, kind="stable") if not dead[g]][:B]
        if len(first) < B or not loader.padded(first):
            raise RuntimeError(f"{name}: the set has no padded batch without a dead-row graph to record a step on")
        index = gs.prepare(first)                      # the static index buffer: every replay reads this address
        c = ops.collate_graphs(gs, index, loader.dtypes, extras=loader.extras, pad=cap, pad_quant=quant)
        b = pyg_lite.attach_batch(c)

        def run():
            ops.collate_graphs(gs, index, loader.dtypes, out=c, extras=loader.extras, pad=cap, pad_quant=quant)
            return run_batch(b)

        accepts(b)
        # (the quantised routes ask ops._workspace for other sizes than the plain ones: their recording is guarded)
        replay = self._capture((), warmup, counters=counters, run=run, guard_workspace=quant)
        counts = gs.counts if gs._sym_norm2 is None else gs.counts + (gs._sym_norm2.counts,)

        def walk(replayed, eager):
            batches = loader.batches()
            recorded = [loader.padded(ids) for ids in batches]
            host = [ops.batch_offsets(counts, ids)[0] for ids, r in zip(batches, recorded) if r]
            if host:
                dev = torch.from_numpy(np.stack(host)).pin_memory().to(gs.device, non_blocking=True)
            k = 0
            for ids, r in zip(batches, recorded):
                if r:
                    index.refill(dev[k], ids)
                    k += 1
                    replayed(replay())
                else:
                    eager(loader.collate(ids))

        return replay, c, walk

    def evaluate(self, x, edge_index, batch, y, n_real=None, into=None):
        """One batch of an evaluation pass -> (totals, loss_sum), device tensors: totals int64 [2] = (graphs, graphs whose
        arg-max class is the label), loss_sum float64 [1] = their summed cross entropy.  into: an EvalSums to ADD to (the
        batches of a pass accumulate on the device; the tensors returned are its own); a fresh zeroed one otherwise.
        n_real: the real graph count of a padded batch (Batch.num_real_graphs); the filler graphs behind them reach no sum.

        The model runs in eval mode (its mode is put back) with gradients off: its fused eval forward up to the pooled
        means (model.eval_pooled), then ops.head_eval -- no logits leave the device, nothing synchronises, and no
        parameter, moment or `t` is touched.  Where the fused route declines a batch the layers run one by one
        (model.layers_pooled) with the same tail, as in step(); a padded batch is refused there with step()'s
        RuntimeError, and so is a batch whose `batch` vector is not sorted (its pooling exists only inside the model's
        forward)."""
        with self._eval_mode() as model:
            pooled = model.eval_pooled(x, edge_index, batch)
            if pooled is None:
                if self._is_padded(batch):
                    raise RuntimeError(f"StackTrainer.evaluate: the fused route declined a padded batch: "
                                       f"{self._declined(batch, training=False)}")
                pooled = model.layers_pooled(x, edge_index, batch)
            if pooled is None:
                raise RuntimeError("StackTrainer.evaluate: `batch` is not sorted (or the kernels are off): the model pools "
                                   "inside its own forward")
            if into is None:
                into = EvalSums(pooled.device)
            pooled = pooled.float().contiguous()
            if n_real is not None and y.shape[0] == n_real < pooled.shape[0]:
                pooled = pooled[:n_real]               # the labels of the real graphs only
            ops.head_eval(pooled, model.lin.weight, model.lin.bias, y, n_real=n_real, totals=into.totals,
                          loss_sum=into.loss_sum)
        return into.totals, into.loss_sum

    def capture_eval_loader(self, loader, warmup=2):
        """ONE recorded evaluation for every padded batch of `loader` (a pyg_lite.GraphLoader(pad=True), shuffled or not)
        -> a callable that runs a whole pass and returns (totals, loss_sum) on the device, as evaluate() gives them.

        The recording is the padded collation (with the cached plans' table launches behind it), the fused eval forward
        and ops.head_eval on the real graphs, adding into one EvalSums -- capture_loader's machinery (_capture_padded)
        around evaluate() in place of step().  A pass zeroes the sums (one launch), replays every padded batch and runs
        the batches that arrive unpadded -- the short last batch among them -- through evaluate() into the same sums:
        every graph of the set is counted exactly once, and the pass equals
        `for b in loader: evaluate(b.x, b.edge_index, b.batch, b.y, b.num_real_graphs, into=sums)` bit for bit.  Nothing
        synchronises; the tensors returned are the pass's own (pass.sums), overwritten by the next pass.  If the model's
        fused eval route declines the padded batch, RuntimeError names the reason: a padded batch never falls back."""
        sums = None

        def accepts(b):
            nonlocal sums
            sums = EvalSums(b.x.device)
            one(b)                                     # raises where the fused route declines the padded batch

        def one(b):
            return self.evaluate(b.x, b.edge_index, b.batch, b.y, b.num_real_graphs, into=sums)

        replay, c, walk = self._capture_padded(loader, warmup, "capture_eval_loader", accepts, one)
        return self._eval_pass(sums, walk, one, (sums.totals, sums.loss_sum), graph=replay.graph, collated=c)


class EvalSums:
    """The accumulators of an evaluation pass, on the device: totals int64 [2] = (graphs, hits) and loss_sum float64 [1],
    views of one 24-byte buffer (`buffer`, int64 [3]: one zero_() clears them, one copy reads them back)."""

    def __init__(self, device):
        self.buffer = torch.zeros(3, dtype=torch.int64, device=device)
        self.totals, self.loss_sum = self.buffer[:2], self.buffer[2:].view(torch.float64)

    def zero_(self):
        self.buffer.zero_()
        return self

    @staticmethod
    def read(*sums):
        """[(graphs, hits, loss_sum)] of several EvalSums on the host, by ONE device-to-host copy (it synchronises)."""
        host = torch.stack([s.buffer for s in sums]).cpu()
        return [(int(row[0]), int(row[1]), float(row[2:].view(torch.float64)[0])) for row in host]


class BestTracker:
    """The reference loop's save-best / load-best step on the device (demo_sgrace.py:583-610: `if test_acc > best_acc:
    torch.save(model.state_dict())`, and `load_state_dict(best)` after the last epoch), without a read-back per epoch.

        tracker = trainer.track_best(epochs=E)
        for epoch in range(E):
            ...                                   # the epoch's steps, then the evaluation passes into their EvalSums
            tracker.update(val_sums, test_sums)   # one ops.keep_best: val_sums decides; nothing synchronises
        best_epoch, best_n, best_hits, done, log = tracker.read()      # ONE device-to-host copy for the whole run
        tracker.restore()                         # the model is the best epoch's again

    It holds one snapshot tensor per trainer.params (initialised to the parameters' current values, so restore() before
    any winning epoch leaves the model as it is), the state int64 [4] = (best_n, best_hits, best_epoch, epoch), fresh as
    (1, 0, -1, 0), and with `epochs` a log of that many rows for up to 4 EvalSums.  The comparison is exact and in
    integers (include/sgx.h, "model selection"): strictly more hits per row wins, a tie keeps the earlier epoch.  The
    optimiser's moments and `t` are neither kept nor restored."""

    def __init__(self, trainer, epochs=None):
        self.trainer = trainer
        self.params = trainer.params
        if len(self.params) > ops._lib.SGX_BEST_MAX_TENSORS:
            raise ValueError(f"BestTracker keeps at most {ops._lib.SGX_BEST_MAX_TENSORS} tensors (the model has {len(self.params)})")
        dev = self.params[0].device
        self.snapshot = [p.detach().clone(memory_format=torch.contiguous_format) for p in self.params]
        self.state = torch.tensor([1, 0, -1, 0], dtype=torch.int64).to(dev)
        self.epochs = None if epochs is None else int(epochs)
        if self.epochs is not None and self.epochs < 0:
            raise ValueError("epochs must not be negative")
        # the log's rows are 3 words per EvalSums; how many there are is known at the first update()
        self._log_words = None if not self.epochs else torch.zeros(self.epochs * 3 * ops._lib.SGX_BEST_MAX_SUMS, dtype=torch.int64,
                                                                   device=dev)
        self.n_sums, self.log = None, None

    def update(self, *sums):
        """One epoch: ops.keep_best on the trainer's parameters with `sums` -- EvalSums (or their int64 [3] buffers), the
        first decides.  Every call of one tracker takes the same number of them.  Does not synchronise and may be called
        inside torch.cuda.graph."""
        buffers = [getattr(s, "buffer", s) for s in sums]
        if self.n_sums is None:
            if not 1 <= len(buffers) <= ops._lib.SGX_BEST_MAX_SUMS:
                raise ValueError(f"update takes 1 to {ops._lib.SGX_BEST_MAX_SUMS} EvalSums (got {len(buffers)})")
            self.n_sums = len(buffers)
            if self._log_words is not None:
                self.log = self._log_words[: self.epochs * 3 * self.n_sums].view(self.epochs, 3 * self.n_sums)
        elif len(buffers) != self.n_sums:
            raise ValueError(f"this tracker's epochs carry {self.n_sums} EvalSums (got {len(buffers)})")
        ops.keep_best(self.params, self.snapshot, buffers, self.state, self.log)

    def restore(self):
        """Copies the snapshot into the parameters, device to device, without a read-back.  The copies are torch's in-place
        ones, so every parameter's version counter moves and whatever is cached by it is rebuilt; the models and trainers
        themselves derive the transposed and quantised weights from the parameters in every forward.  The moments and `t`
        are not touched."""
        with torch.no_grad():
            for p, s in zip(self.params, self.snapshot):
                p.copy_(s)

    def read(self):
        """(best_epoch, best_n, best_hits, epochs_done, log) by ONE device-to-host copy (it synchronises): best_epoch is
        -1 while no epoch has won; log holds, per logged epoch, [(n, hits, loss_sum), ...] in the order update() took the
        sums -- the epochs done, as far as the log's rows go; empty without `epochs`."""
        words = self.state if self.log is None else torch.cat([self.state, self.log.reshape(-1)])
        host = words.cpu()
        best_n, best_hits, best_epoch, done = (int(v) for v in host[:4])
        rows = host[4:].view(-1, 3) if self.log is not None else host[4:]
        log = []
        for e in range(min(done, self.epochs or 0) if self.log is not None else 0):
            row = rows[e * self.n_sums:(e + 1) * self.n_sums]
            log.append([(int(r[0]), int(r[1]), float(r[2:].view(torch.float64)[0])) for r in row])
        return best_epoch, best_n, best_hits, done, log

    def state_dict(self):
        """The snapshot under the model's parameter names (clones; parameters the trainer does not train are left out)."""
        names = {id(p): name for name, p in self.trainer.model.named_parameters()}
        return {names[id(p)]: s.clone() for p, s in zip(self.params, self.snapshot)}


class NodeTrainer(_Trainer):
    """Adam on the kernels for sgrace.GAT_PYNQ, the node classifier of the demo.

        trainer = NodeTrainer(model, lr=0.01, weight_decay=5e-4)
        loss = trainer.step(x, edge_index, y, mask=train_mask)            # full graph: a device tensor [1]
        loss = trainer.step(b.x, b.edge_index_agg, b.y, n_prefix=b.batch_size)      # a seeds-first mini-batch
        counts, loss = trainer.evaluate(x, edge_index, y, test_mask)      # device int64 [selected, hits], device loss [1]
        replay = trainer.capture(x, edge_index, y, train_mask)            # the full-graph step, recorded once
        epoch = trainer.capture_loader(loader)                            # a NeighborLoader(pad=True): one recorded step for every full batch
        sums = trainer.evaluate(b.x, b.edge_index_agg, b.y, n_prefix=b.batch_size, into=sums)      # ADDS the batch to an EvalSums
        test = trainer.capture_eval_loader(test_loader)                   # a NeighborLoader(pad=True): one recorded evaluation
        (rows, hits, loss_sum), = EvalSums.read(test())                   # one pass over the loader's nodes, one read-back

    A step is model.features -> ops.NodeLoss on the device counter `t` -> loss.backward() through the layers' own autograd
    -> one ops.adam_step over every parameter that received a gradient (the layers' never-used `bias` parameters receive
    none and are skipped, as torch skips them).  The rows that count are `mask` (bool [n]) and / or the first `n_prefix`
    rows; how many they are is counted on the device, so a step synchronises nothing of its own.  The dropout stream is
    ops.node_loss's counter-based mask of (seed, t), not torch's generator; the layers run in whatever mode the model is in."""

    def __init__(self, model, lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, p_drop=0.5, seed=12345):
        if not hasattr(model, "features") or not hasattr(model, "lin"):
            raise TypeError("NodeTrainer takes a GAT_PYNQ")
        super().__init__(model, lr, betas, eps, weight_decay, p_drop, seed)

    def step(self, x, edge_index, y, mask=None, n_prefix=None):
        model = self.model
        for p in self.params:
            p.grad = None
        H = model.features(x, edge_index).contiguous()
        loss = ops.NodeLoss.apply(H, model.lin.weight, model.lin.bias, y, mask, n_prefix, self.p_drop, self.seed, 0, self.t)
        loss.backward()
        self._adam([p.grad for p in self.params])
        return loss.detach().reshape(1)

    def evaluate(self, x, edge_index, y, mask=None, n_prefix=None, into=None):
        """(counts, loss) of the selected rows in eval mode without dropout: counts = device int64 [selected rows, rows
        whose arg-max class is the target], loss their mean.  No logits leave the device; the model's mode is put back.

        into: an EvalSums to ADD this batch to, for a pass over a loader -- the same features, then ops.node_eval in place
        of ops.node_loss: totals += (selected rows, hits), the hits that `counts` holds without it, and loss_sum += the
        rows' summed loss in double.  Returns `into`.  Nothing synchronises, and no parameter, moment or `t` is touched."""
        with self._eval_mode() as model:
            H = model.features(x, edge_index).contiguous()
            if into is not None:
                ops.node_eval(H, model.lin.weight, model.lin.bias, y, into.totals, into.loss_sum, mask=mask, n_prefix=n_prefix)
                return into
            loss, _, _, _, counts = ops.node_loss(H, model.lin.weight, model.lin.bias, y, mask=mask, n_prefix=n_prefix, p=0.0,
                                                  want_counts=True, grads=False)
        return counts, loss

    def _configuration(self):
        from . import config
        return (f"compute_attention={config.compute_attention} accb={config.accb} fake_quantization={config.fake_quantization} "
                f"hardware_quantize={config.hardware_quantize} gat_edge_outputs={config.gat_edge_outputs} "
                f"float_type={getattr(config.float_type, '__name__', config.float_type)}")

    def capture(self, x, edge_index, y, mask=None, n_prefix=None, warmup=2):
        """Record the full-graph step with torch.cuda.graph (one stream) and return a callable that replays it and returns
        the loss tensor the replay fills.  The warm-up steps (they build what a step caches: the CSRs, the plans, the
        workspaces) run on a copy of the state, which is put back before the capture: n replays equal n eager steps.  The
        last warm-up step runs under torch.cuda.set_sync_debug_mode("error"): a layer path that synchronises cannot be
        captured, and capture() raises a RuntimeError that names the configuration instead of recording it."""
        batch = (x, edge_index, y, mask, n_prefix)
        return self._capture(batch, warmup, self._sync_probe("capture", lambda: self.step(*batch)))

    def _sync_probe(self, name, run):
        """The probe of capture() and capture_loader(): run() once more under torch.cuda.set_sync_debug_mode("error") ->
        None, or the RuntimeError to raise in place of recording a step that synchronises."""
        def probe():
            mode = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                run()
            except RuntimeError as e:
                if "synchroniz" not in str(e):        # torch's sync-debug message; any other error is the caller's to see
                    raise
                failure = RuntimeError(f"NodeTrainer.{name}: the layer path synchronises with {self._configuration()}; "
                                       f"the step is not captured ({e})")
                failure.__cause__ = e
                return failure
            finally:
                torch.cuda.set_sync_debug_mode(mode)

        return probe

    def capture_loader(self, loader, warmup=2):
        """ONE recorded step for every full batch of `loader` (a pyg_lite.NeighborLoader(pad=True); anything else:
        ValueError) -> a callable that runs one epoch and returns its losses, one device tensor [1] per batch, in the
        loader's order.

        The recorded step is the padded sample and its preparation (loader.padded_batch(): sgx_node_batch_sample_padded
        into the loader's one set of buffers, the gather of x and, with transposed=True, the transposes), model.features,
        ops.NodeLoss with n_prefix = batch_size, the layers' backward and ops.adam_step -- one stream, no parallel
        branches, as capture().  An epoch draws its batches as iterating the loader would; per full batch the seeds and the
        step word are copied into the loader's fixed buffers (loader.load: device to device, no synchronisation) and the
        recording is replayed; the short last batch runs through step() unpadded in its place.  An epoch thus takes
        exactly the steps of `for b in loader: step(b.x, b.edge_index_agg, b.y, n_prefix=b.batch_size)`, bit for bit.
        Covers GAT_PYNQ with config.compute_attention 0 and 1 (attention needs a transposed=True loader: the backward's
        transposed pattern is then built on the device), config.gat_edge_outputs 1 and 0, fp32 and fp16, config.accb = 0
        -- and config.accb = 1 from a loader with schedule="flat" and transposed=True, whose adjacency, X and X^T the one-call
        backward takes on its entry-split schedules (no plan, no read-back);
        and the quantised model -- config.fake_quantization with and without config.hardware_quantize, fp32 -- from a
        loader with quant= (NeighborLoader(pad=True, quant=qc): the padded batch carries the quantised adjacencies of both
        layers with their constant facts and lean mask values, sgx_node_batch_sample_padded_quant, so the quantised layers
        launch no quantiser for the adjacency and read nothing back).  The warm-up steps run on the
        loader's first batch_size input nodes on a copy of the state; the last of them runs under
        torch.cuda.set_sync_debug_mode("error"), and a configuration whose layer path synchronises raises capture()'s
        RuntimeError instead of being recorded.  loader.status() tells, once per epoch or run, whether a batch failed."""
        one = lambda b: self.step(b.x, b.edge_index_agg, b.y, n_prefix=b.batch_size)
        replay, walk = self._capture_padded(loader, warmup, "capture_loader", "a step", one, backward=True)

        def epoch():
            losses = []
            walk(lambda loss: losses.append(loss.clone()), lambda b: losses.append(one(b)))
            return losses

        epoch.graph, epoch.replay = replay.graph, replay
        return epoch

    def _capture_padded(self, loader, warmup, name, what, run_batch, backward=False):
        """What capture_loader and capture_eval_loader share: ONE recording of run_batch(b) on the padded batch b of
        `loader` (a pyg_lite.NeighborLoader(pad=True) with labels; anything else: ValueError) behind its sample and
        preparation (loader.padded_batch()) -> (replay, walk).  The warm-up runs on the loader's first batch_size input
        nodes, the last of them through _sync_probe.  backward: what is recorded runs the layers' backward, which with
        config.compute_attention needs a transposed=True loader.  walk(replayed, eager) takes one pass over the loader as
        iterating it would (loader.epoch_batches()): per full batch the seeds and the step word are copied into the
        loader's fixed buffers (loader.load), the recording is replayed and replayed(what run_batch returned) called; the
        short last batch is drawn unpadded and handed to eager(batch) in its place."""
        from . import config
        if not getattr(loader, "pad", False) or not hasattr(loader, "padded_batch"):
            raise ValueError(f"{name} takes a NeighborLoader(pad=True)")
        if backward and int(config.compute_attention) and not loader.transposed:
            raise ValueError(f"{name}: with config.compute_attention the loader needs transposed=True (the backward "
                             "would otherwise build the transposed pattern with a sort, per batch)")
        if loader.y is None:
            raise ValueError(f"{name}: the loader's data carries no labels")
        B = loader.capacity.batch_size
        if loader.input_nodes.numel() < B:
            raise RuntimeError(f"{name}: the loader has no full batch to record {what} on")
        loader.load(loader.input_nodes[:B], 0)
        run = lambda: run_batch(loader.padded_batch())
        replay = self._capture((), warmup, self._sync_probe(name, run), run=run)

        def walk(replayed, eager):
            for seeds, input_id, step in loader.epoch_batches():
                if loader.padded(seeds):
                    loader.load(seeds, step)
                    replayed(replay())
                else:
                    eager(loader._batch(seeds, input_id, step))

        return replay, walk

    def capture_eval_loader(self, loader, warmup=2):
        """ONE recorded evaluation for every full batch of `loader` (a pyg_lite.NeighborLoader(pad=True), shuffled or not;
        anything else, or a loader without labels: ValueError) -> a callable that runs a whole pass over the loader's input
        nodes and returns its EvalSums (pass.sums: the selected rows, the hits and the summed loss, on the device).

        The recording is the padded sample and its preparation (loader.padded_batch(), into the loader's one set of
        buffers), model.features in eval mode and ops.node_eval with n_prefix = batch_size, adding into one EvalSums -- one
        stream, no parallel branches: capture_loader's machinery (_capture_padded) around evaluate(into=) in place of
        step().  A pass zeroes the sums (one launch), draws its batches as iterating the loader would, per full batch copies
        the seeds and the step word into the loader's fixed buffers and replays, and runs the short last batch through
        evaluate(into=) unpadded: every input node is counted exactly once, and the pass equals
        `for b in loader: evaluate(b.x, b.edge_index_agg, b.y, n_prefix=b.batch_size, into=sums)` bit for bit.  Nothing
        synchronises: EvalSums.read(pass(), ...) reads one or several passes back in one copy; the sums are the pass's
        own, overwritten by the next pass.  Parameters, moments and `t` are untouched and the model's mode is put back.
        The forward reads no transposed pattern, so transposed=True is not needed.  Covers what capture_loader covers: GCN
        and attention, config.gat_edge_outputs 1 and 0, config.accb = 0 (and 1 from a schedule="flat" loader: the forward
        does not read the flag), and the quantised model (config.fake_quantization
        with and without config.hardware_quantize) from a loader with quant=.  The last warm-up evaluation runs under
        torch.cuda.set_sync_debug_mode("error"): a configuration whose layer path synchronises raises capture()'s
        RuntimeError instead of being recorded.  A loader shared with capture_loader shares its buffers: a padded batch
        is valid until the next one is drawn, so passes and training epochs run one after the other, never interleaved
        batch by batch on one loader.  loader.status() tells, once per epoch or run, whether a batch failed."""
        def one(b):
            return self.evaluate(b.x, b.edge_index_agg, b.y, n_prefix=b.batch_size, into=sums)

        sums = EvalSums(self.t.device)
        replay, walk = self._capture_padded(loader, warmup, "capture_eval_loader", "an evaluation", one)
        return self._eval_pass(sums, walk, one, sums, graph=replay.graph, replay=replay)
