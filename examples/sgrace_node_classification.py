#!/usr/bin/env python3
"""Node classification with the SGRACE library's layers on the GPU kernels -- the call pattern of
the reference's demo (demo/emulation/demo_sgrace.py: init_SGRACE, GAT_PYNQ, train / test), on a
synthetic planted-partition graph because the demo's datasets (Planetoid Cora, Amazon Photo) are
downloaded by torch_geometric and are not available offline.

    python examples/sgrace_node_classification.py [--attention [--lean-gat]] [--qbits 8] [--epochs 60] [--acc 0]
                                                  [--batch-size 128 --num-neighbors 10,10 [--device-batches]] [--accb]
                                                  [--trainer [--replay] [--keep-best]]

--attention  GAT edge softmax instead of the GCN aggregate (config.compute_attention)
--lean-gat   with --attention on the kernels: the forward keeps the row softmax statistics instead of the per-edge outputs
             E and S, and the backward forms them again (config.gat_edge_outputs = 0: 3 n + n_cols floats per layer
             in place of 2 nnz)
--accb       on the kernels: every layer's backward as one call of the C ABI (config.accb = 1, sgx_layer_backward) instead
             of the stage calls the autograd function composes; the same arithmetic
--seed S     the seed of the graph, the split and the initial weights
--qbits B    run the layers with the quantised arithmetic of the SGRACE bitstream (config.fake_quantization and
             config.hardware_quantize, as the reference's board configs set them: integer operands on the int8 matrix
             cores for the dense-feature layer when it is wider than 128 columns -- --hidden 256 makes layer 2 such a layer)
--emulate    with --qbits: config.fake_quantization only (the fp32 emulation of the grid everywhere)
--acc 0      the reference's dense torch emulation instead of the kernels (small graphs only)
--batch-size B --num-neighbors K1[,K2..]
             the demo's mini-batch mode (demo_sgrace.py:112-125, full_graph = 0): every epoch trains on
             pyg_lite.NeighborLoader batches of B training nodes with K1 sampled neighbours per node at hop 1, K2 at
             hop 2 ..., sampled on the GPU; evaluation stays on the full graph
--device-batches
             with --batch-size: the loader hands over layer-ready batches (NeighborLoader(..., prepare="sym_norm2")): the
             normalised adjacency, the feature CSR, the labels and masks are built on the GPU behind the sample, and a
             training step synchronises once, inside the sampler; with --accb or --attention the batches also carry
             the transposed matrices the backward reads (transposed=True: X^T for grad_weights over CSR features, the
             transposed pattern of the GAT backward), built on the GPU by sgx_csr_transpose instead of a sort per batch;
             with --qbits the batches also carry the quantised adjacency of both layers with its dead-row facts
             (quant=sgrace.quant_constants), so the quantised layers too launch nothing and read nothing back for it
--trainer    on the kernels: the tail of every step -- dropout, the Linear head, the cross entropy over the training rows,
             their gradients and Adam -- as train.NodeTrainer runs it (sgx_node_loss, sgx_adam_step) instead of torch's;
             the plain mini-batch mode hands batch.train_mask over as the mask (no boolean index, no read-back per step),
             and the final accuracies are counted on the device (NodeTrainer.evaluate); with --batch-size and
             --device-batches (no --accb; with --qbits the loaders carry the quantised adjacency too) every epoch also
             ends as the demo's does, with test(loader, split):
             the nodes outside the training set are split into a validation and a test set, each with a NeighborLoader of
             its own, a pass over each sums hits and loss on the device (NodeTrainer.evaluate(into=), sgx_node_eval) and
             both sets' sums are read back in one transfer; test_acc is then the sampled test accuracy -- hits over
             selected rows -- of the epoch that validated best
--replay    with --trainer on the full graph: the whole step captured once (torch.cuda.graph) and replayed every epoch;
             with --batch-size, --num-neighbors and --device-batches: the loader pads every full batch to one fixed
             capacity (NeighborLoader(pad=True)) and ONE recorded step -- sample, preparation, layers, loss, backward,
             Adam -- is replayed for each of them (NodeTrainer.capture_loader); the short last batch runs eager; the
             validation and test passes are replayed the same way, ONE recorded evaluation per padded loader
             (NodeTrainer.capture_eval_loader); with --qbits the padded batches carry the quantised adjacency of both
             layers (NeighborLoader(pad=True, quant=sgrace.quant_constants)) and the recorded step and evaluations are the
             quantised model's; --accb is an eager route except with --flat, whose batches sgx_layer_backward takes
             entry-split
--keep-best  with --trainer, --batch-size and --device-batches (no --accb), where every epoch ends with the validation and
             test passes: the demo's save-best / load-best step on the device (train.BestTracker, sgx_keep_best).  Every
             epoch ends with one call that compares the validation counts with the best so far in integers, keeps a copy
             of the weights where the epoch wins and logs both passes' sums; nothing is read back per epoch (with --replay
             the loop runs under torch.cuda.set_sync_debug_mode("error")).  After the last epoch the run is read back in
             ONE transfer, the best epoch's weights are put back and both passes run once more on the samples of that
             epoch: restored_test_acc, which equals that epoch's logged test accuracy; the final train_acc is then the
             restored model's
--flat      with --trainer, --batch-size and --device-batches: the padded loaders deliver their
             batches for the entry-split schedule (NeighborLoader(pad=True, schedule="flat")): every CSR of a batch is
             marked with_facts(flat=True), the layers aggregate by stored entries (SGX_SCHEDULE_FLAT) and build no plan, so
             fan-outs over 63 (--num-neighbors 100,10), feature rows over 64 entries and capacities past 2^20 entries
             pad -- and, with --replay, record -- like any other; with --accb every layer's backward is the one call on
             the same schedule (sgx_layer_grad_desc.schedule_adj / _fea / _xt), X and X^T delivered flat-marked by the
             loader (transposed=True), and records and replays as well; with --qbits (no --accb) the loaders take the
             quantised layers' opt-in as well (NeighborLoader(..., quant=qc, flat_quant=True)): the quantised adjacencies
             arrive at capacity, marked with_facts(flat=True, flat_quant=True), and the quantised model -- the demo's
             default arithmetic -- pads and records at those fan-outs too
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def planted_partition(n, classes, f_in, p_in, p_out, seed, device):
    """Labels, an undirected edge list denser inside classes, and non-negative features in [0, 1]
    (the range the quantiser tables assume) that carry a weak class signal."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, classes, (n,), generator=g)
    same = y[:, None] == y[None, :]
    prob = torch.where(same, torch.tensor(p_in), torch.tensor(p_out))
    upper = torch.triu(torch.rand((n, n), generator=g) < prob, diagonal=1)
    src, dst = upper.nonzero(as_tuple=True)
    edge_index = torch.stack([torch.cat([src, dst]), torch.cat([dst, src])])
    proto = (torch.rand((classes, f_in), generator=g) < 0.15).float()
    x = ((torch.rand((n, f_in), generator=g) < 0.04).float() + proto[y] * (torch.rand((n, f_in), generator=g) < 0.25)).clamp(0, 1)
    return x.to(device), edge_index.to(device), y.to(device)


def run(attention=False, qbits=32, epochs=60, acc=1, n=3000, hidden=16, seed=1, verbose=True, emulate=False,
        batch_size=None, num_neighbors=None, lean_gat=False, device_batches=False, accb=0, trainer=False,
        replay=False, keep_best=False, flat=False):
    from sgracex1_amd import config, sgrace
    config.acc = acc
    config.accb = int(accb)
    config.gat_edge_outputs = 0 if lean_gat else 1
    config.compute_attention = int(attention)
    config.fake_quantization = int(qbits != 32)
    config.hardware_quantize = int(qbits != 32 and not emulate)
    config.w_qbits = qbits
    config.float_type = np.float32
    device = torch.device("cuda" if acc == 1 else "cpu")
    config.device = str(device)
    sgrace.init_SGRACE()
    torch.manual_seed(seed)
    x, edge_index, y = planted_partition(n, 5, 200, 0.02, 0.002, seed, device)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).to(device)
    train, test = perm[: n // 5], perm[n // 5:]
    model = sgrace.GAT_PYNQ(x.shape[1], hidden, 1, 5).to(device)
    node_trainer = replay_step = None
    if trainer:
        from sgracex1_amd.train import NodeTrainer
        node_trainer = NodeTrainer(model, lr=0.01, weight_decay=5e-4, seed=seed)
        full_mask = torch.zeros(n, dtype=torch.bool, device=device)
        full_mask[train] = True
    else:
        opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4)
        crit = torch.nn.CrossEntropyLoss()
    loader = None
    if batch_size:
        from sgracex1_amd import pyg_lite
        train_mask = torch.zeros(n, dtype=torch.bool, device=device)
        train_mask[train] = True
        data = pyg_lite.NodeData(x, edge_index, y, train_mask=train_mask)
        ready = {"prepare": "sym_norm2", "transposed": bool(accb or attention), "quant": sgrace.quant_constants}
        if replay or flat:
            ready["pad"] = True
        if flat:
            ready["schedule"] = "flat"
            ready["flat_quant"] = sgrace.quant_constants is not None
        loader = pyg_lite.NeighborLoader(data, num_neighbors or [10], batch_size=batch_size, input_nodes=train_mask,
                                         shuffle=True, seed=seed, **(ready if device_batches else {}))
    passes = None
    if loader is not None and node_trainer is not None and device_batches and (not accb or flat):
        # the demo's test(loader, split) every epoch (demo_sgrace.py:509-601), summed on the device: the nodes outside the
        # training set are split into a validation and a test set with a loader each; an epoch ends with a pass over both
        # (NodeTrainer.evaluate(into=); with --replay ONE recorded evaluation per loader, NodeTrainer.capture_eval_loader)
        # and reads both sets' sums back in one transfer
        from sgracex1_amd.train import EvalSums
        val, test = test[: n // 5], test[n // 5:]
        passes = []
        for nodes in (val, test):
            ev = pyg_lite.NeighborLoader(data, num_neighbors or [10], batch_size=batch_size, input_nodes=nodes, shuffle=False,
                                         seed=seed, prepare="sym_norm2", quant=sgrace.quant_constants, pad=bool(replay or flat),
                                         schedule="flat" if flat else None,
                                         flat_quant=bool(flat and sgrace.quant_constants is not None))
            if replay and nodes.numel() >= batch_size:
                passes.append((ev, node_trainer.capture_eval_loader(ev)))
            else:
                def eager(ev=ev, sums=EvalSums(device)):
                    sums.zero_()
                    for b in ev:
                        node_trainer.evaluate(b.x, b.edge_index_agg, b.y, n_prefix=b.batch_size, into=sums)
                    return sums
                passes.append((ev, eager))
    tracker = None
    if keep_best:
        if passes is None:
            raise ValueError("keep_best needs the per-epoch passes: trainer, batch_size, device_batches, no accb")
        tracker = node_trainer.track_best(epochs)
        first_pass = [ev.epoch for ev, _ in passes]         # the epoch number (it seeds the samples) of every loader's first pass
        if replay:
            replay_step = node_trainer.capture_loader(loader)
            sync_mode = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")         # from the first epoch to the last nothing may synchronise
    best_val, test_at_best = -1.0, 0.0
    printed = []
    t0 = time.time()
    epoch_loss = []                                         # mean training loss of every epoch, kept on the device
    for epoch in range(epochs):
        model.train()
        total, steps = 0, 0
        if loader is None and node_trainer is not None:
            if replay and replay_step is None:
                replay_step = node_trainer.capture(x, edge_index, y, full_mask)
            loss = replay_step() if replay else node_trainer.step(x, edge_index, y, full_mask)
            total, steps = loss[0], 1
        elif node_trainer is not None and replay:
            if replay_step is None:
                replay_step = node_trainer.capture_loader(loader)
            for loss in replay_step():
                total, steps = total + loss[0], steps + 1
        elif node_trainer is not None:
            for batch in loader:
                if device_batches:
                    loss = node_trainer.step(batch.x, batch.edge_index_agg, batch.y, n_prefix=batch.batch_size)
                else:
                    loss = node_trainer.step(batch.x, batch.edge_index.flip(0), batch.y, mask=batch.train_mask)
                total, steps = total + loss[0], steps + 1
        elif loader is None:
            opt.zero_grad()
            loss = crit(model(x, edge_index)[train], y[train])
            loss.backward()
            opt.step()
            total, steps = loss.detach(), 1
        else:
            for batch in loader:                            # demo_sgrace.py train(), :476-507
                opt.zero_grad()
                # the layers aggregate at edge_index[0]; PyG's batches put the seed in row 1, so flipped, each seed row
                # holds its sampled neighbours (taken literally, it would hold its self loop and little else)
                if device_batches:
                    # edge_index_agg is that flipped list with the normalised CSR attached; the seeds are rows
                    # 0 .. batch_size-1 and every input node is a training node, so no mask (and no sync) is needed
                    out = model(batch.x, batch.edge_index_agg)
                    loss = crit(out[:batch.batch_size], batch.y[:batch.batch_size])
                else:
                    out = model(batch.x, batch.edge_index.flip(0))
                    loss = crit(out[batch.train_mask], batch.y[batch.train_mask])
                loss.backward()
                opt.step()
                total, steps = total + loss.detach(), steps + 1
        epoch_loss.append(total / max(steps, 1))
        if tracker is not None:
            tracker.update(*[run_pass() for _, run_pass in passes])      # validation decides; nothing is read back
        elif passes is not None:
            (m_val, hit_val, _), (m_te, hit_te, _) = EvalSums.read(*[run_pass() for _, run_pass in passes])
            if hit_val / m_val > best_val:                  # the test accuracy of the epoch that validates best
                best_val, test_at_best = hit_val / m_val, hit_te / m_te
        if verbose and (epoch + 1) % 20 == 0:
            if tracker is not None:
                printed.append((epoch, loss.detach().clone()))       # printed behind the loop
            else:
                print(f"epoch {epoch + 1:3d}  loss {float(loss):.4f}", flush=True)
    if tracker is not None and replay:
        torch.cuda.set_sync_debug_mode(sync_mode)
    if loader is not None and replay:
        for ld in [loader] + [ev for ev, _ in passes or []]:
            ld.status()                                     # what a failed batch would have raised, read back once
    if device.type == "cuda":
        torch.cuda.synchronize()
    elapsed = time.time() - t0
    kept = {}
    if tracker is not None:
        best_epoch, _, _, _, log = tracker.read()           # the whole run in ONE device-to-host copy
        for epoch, loss in printed:
            print(f"epoch {epoch + 1:3d}  loss {float(loss):.4f}", flush=True)
        epoch_acc = [[hits / n for n, hits, _ in row] for row in log]
        test_at_best = epoch_acc[best_epoch][1] if best_epoch >= 0 else 0.0
        tracker.restore()                                   # the demo's load_state_dict(best)
        for (ev, _), first in zip(passes, first_pass):
            ev.epoch = first + max(best_epoch, 0)           # the passes of the best epoch drew their samples from this number
        _, (m_te, hit_te, _) = EvalSums.read(*[run_pass() for _, run_pass in passes])
        kept = {"best_epoch": best_epoch, "restored_test_acc": hit_te / m_te, "epoch_acc": epoch_acc}
    model.eval()
    if node_trainer is not None:
        (m_tr, hit_tr), (m_te, hit_te) = (node_trainer.evaluate(x, edge_index, y, m)[0].tolist() for m in (full_mask, ~full_mask))
        train_acc, test_acc = hit_tr / m_tr, hit_te / m_te
        if passes is not None:
            test_acc = test_at_best
    else:
        with torch.no_grad():
            pred = model(x, edge_index).argmax(1)
        train_acc, test_acc = float((pred[train] == y[train]).float().mean()), float((pred[test] == y[test]).float().mean())
    result = {"train_acc": train_acc, "test_acc": test_acc,
              "edges": int(edge_index.shape[1]), "ms_per_epoch": 1000 * elapsed / epochs,
              "epoch_loss": [float(v) for v in epoch_loss], **kept}
    if loader is not None:
        result["batches_per_epoch"] = len(loader)
    if verbose:
        print(result)
    return result, model, (x, edge_index, y)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--attention", action="store_true")
    ap.add_argument("--qbits", type=int, default=32, choices=[32, 8, 4, 2, 1])
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--acc", type=int, default=1, choices=[0, 1])
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--nodes", type=int, default=3000)
    ap.add_argument("--emulate", action="store_true")
    ap.add_argument("--batch-size", type=int, default=None)
    ap.add_argument("--num-neighbors", type=lambda s: [int(k) for k in s.split(",")], default=None)
    ap.add_argument("--lean-gat", action="store_true")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device-batches", action="store_true")
    ap.add_argument("--accb", action="store_true")
    ap.add_argument("--trainer", action="store_true")
    ap.add_argument("--replay", action="store_true")
    ap.add_argument("--keep-best", action="store_true")
    ap.add_argument("--flat", action="store_true")
    a = ap.parse_args()
    if (a.batch_size is None) != (a.num_neighbors is None) or (a.batch_size is not None and a.acc != 1):
        ap.error("--batch-size and --num-neighbors go together, on the kernels (--acc 1)")
    if a.device_batches and a.batch_size is None:
        ap.error("--device-batches selects the loader of the mini-batch mode (--batch-size, --num-neighbors)")
    if a.trainer and a.acc != 1:
        ap.error("--trainer runs the tail on the kernels (--acc 1)")
    if a.replay and (not a.trainer or (a.batch_size is not None and not a.device_batches)):
        ap.error("--replay replays the step of --trainer: the full-graph one, or the padded mini-batch one of --device-batches")
    if a.replay and a.batch_size is not None and a.accb and not a.flat:
        ap.error("--replay on mini-batches covers the layers with the staged backward, quantised or not (--accb only with --flat)")
    if a.keep_best and not (a.trainer and a.batch_size is not None and a.device_batches and not a.accb):
        ap.error("--keep-best needs --trainer with the per-epoch passes: --batch-size, --num-neighbors, --device-batches, no --accb")
    if a.flat and not (a.trainer and a.batch_size is not None and a.device_batches):
        ap.error("--flat needs --trainer with --batch-size, --num-neighbors and --device-batches")
    if a.flat and a.qbits != 32 and a.accb:
        ap.error("--flat with --qbits runs the staged backward: the one-call backward of a quantised layer keeps the row schedule")
    run(a.attention, a.qbits, a.epochs, a.acc, n=a.nodes, hidden=a.hidden, emulate=a.emulate, batch_size=a.batch_size,
        num_neighbors=a.num_neighbors, lean_gat=a.lean_gat, seed=a.seed, device_batches=a.device_batches,
        accb=int(a.accb), trainer=a.trainer, replay=a.replay, keep_best=a.keep_best, flat=a.flat)
