"""A training step without torch in its tail: StackTrainer runs

    the model's fused stack (one forward launch)  ->  ops.head_loss (dropout, head, cross entropy and every gradient)
    ->  the stack's backward (one launch and a reduction)  ->  ops.adam_step (every parameter, one launch)

on a device step counter that both the dropout mask and Adam's bias corrections read, so the whole step of a fixed batch
can be captured once (torch.cuda.graph) and replayed: the regime of the notebook, one 188-graph batch for 60 steps.

NodeTrainer is the same for node classification (sgrace.GAT_PYNQ): the model's two layers through their own autograd,
ops.NodeLoss (the tail over the selected rows, the count of which never leaves the device) and ops.adam_step.
"""
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

    def _capture(self, batch, warmup, probe=None, counters=()):
        """Record self.step(*batch) with torch.cuda.graph (one stream, no parallel branches) and return a callable that
        replays it and returns the loss tensor the replay fills.  The warm-up steps it needs first (they build what a step
        caches: the CSRs, the plans, the workspaces) run on a side stream on a copy of the state, which is put back before
        the capture: the trainer is where it was, and n replays equal n eager steps.  probe: run on the side stream after
        the warm-up steps; what it returns is raised once the state is back.  counters: the names of host-side counts that
        the recorded step (which computes nothing until it is replayed) must leave as the warm-up left them."""
        saved = self.state()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                self.step(*batch)
            failure = probe() if probe is not None else None
        torch.cuda.current_stream().wait_stream(side)
        self.load_state(saved)
        for p in self.params:
            p.grad = None
        if failure is not None:
            raise failure
        kept = [(name, getattr(self, name)) for name in counters]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss = self.step(*batch)
        for name, value in kept:
            setattr(self, name, value)

        def replay():
            graph.replay()
            return loss

        replay.graph = graph
        return replay


class StackTrainer(_Trainer):
    """Adam on the kernels for GCN_PYNQ(train_stack=True) / GAT_POOL_PYNQ(train_stack=True) (fake quantisation included).

        trainer = StackTrainer(model, lr=0.01)
        loss = trainer.step(x, edge_index, batch, y)          # a device tensor [1]; nothing synchronises
        replay = trainer.capture(x, edge_index, batch, y)     # the step of this batch, recorded once
        loss = replay()

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

    def step(self, x, edge_index, batch, y):
        model = self.model
        for p in self.params:
            p.grad = None
        head = {id(model.lin.weight): None, id(model.lin.bias): None}
        pooled = model.train_pooled(x, edge_index, batch)
        if pooled is not None:
            loss, grad_pooled, grad_w, grad_b = ops.head_loss(pooled, model.lin.weight, model.lin.bias, y, p=self.p_drop,
                                                              seed=self.seed, step=0, step_dev=self.t)
            pooled.backward(grad_pooled)
            head = {id(model.lin.weight): grad_w, id(model.lin.bias): grad_b}
            self.fused_steps += 1
        else:
            pooled = model.layers_pooled(x, edge_index, batch)
            if pooled is not None:
                # the layers one by one with their own autograd; the tail is still the one call, on the same mask stream
                loss = ops.HeadLoss.apply(pooled, model.lin.weight, model.lin.bias, y, self.p_drop, self.seed, 0, self.t)
            else:
                loss = F.cross_entropy(self._forward(x, edge_index, batch), y)
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


class NodeTrainer(_Trainer):
    """Adam on the kernels for sgrace.GAT_PYNQ, the node classifier of the demo.

        trainer = NodeTrainer(model, lr=0.01, weight_decay=5e-4)
        loss = trainer.step(x, edge_index, y, mask=train_mask)            # full graph: a device tensor [1]
        loss = trainer.step(b.x, b.edge_index_agg, b.y, n_prefix=b.batch_size)      # a seeds-first mini-batch
        counts, loss = trainer.evaluate(x, edge_index, y, test_mask)      # device int64 [selected, hits], device loss [1]
        replay = trainer.capture(x, edge_index, y, train_mask)            # the full-graph step, recorded once

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

    def evaluate(self, x, edge_index, y, mask=None, n_prefix=None):
        """(counts, loss) of the selected rows in eval mode without dropout: counts = device int64 [selected rows, rows
        whose arg-max class is the target].  No logits leave the device; the model's mode is put back."""
        model = self.model
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                H = model.features(x, edge_index).contiguous()
                loss, _, _, _, counts = ops.node_loss(H, model.lin.weight, model.lin.bias, y, mask=mask, n_prefix=n_prefix, p=0.0,
                                                      want_counts=True, grads=False)
        finally:
            model.train(was_training)
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

        def probe():
            mode = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                self.step(*batch)
            except RuntimeError as e:
                if "synchroniz" not in str(e):        # torch's sync-debug message; any other error is the caller's to see
                    raise
                failure = RuntimeError(f"NodeTrainer.capture: the layer path synchronises with {self._configuration()}; "
                                       f"the step is not captured ({e})")
                failure.__cause__ = e
                return failure
            finally:
                torch.cuda.set_sync_debug_mode(mode)

        return self._capture(batch, warmup, probe)
