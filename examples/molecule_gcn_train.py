#!/usr/bin/env python3
"""jupyter/molecule_gcn/Graph_Classification.ipynb end to end on the GPU kernels (cells 4-20):
MUTAG (raw TU files from the reference, as committed under tests/golden/), shuffle with seed 12345,
train on all 188 graphs in one batch, test on graphs [50:100], hidden 64, Adam lr 0.01, cross
entropy, fp16 layer kernels in forward, device kernels in backward.  The notebook's recorded run
reaches test accuracy 0.76 at epoch 34 (README.md:126: "0.76 accuracy around epoch 36").

    python examples/molecule_gcn_train.py [--epochs 60] [--acc 0] [--layer-count 2 [--train-stack]]
        --acc 0 = the torch twin; --layer-count 2 = the accuracy passes (eval) run the whole model in one call
        (register layer_count, sgx_stack_forward); training steps run layer by layer unless --train-stack, which
        (with --layer-count >= 2) runs each step's two layers and the pooling as one forward call (sgx_stack_forward)
        and one backward call (sgx_stack_backward) -- GCN_PYNQ(train_stack=True)
    python examples/molecule_gcn_train.py --batch-size 64 [--host-loader] [--layer-count 2 --train-stack]
        --batch-size N > 0 = train the PyG way, on shuffled mini-batches of N graphs (MOL cell 10's
        DataLoader(shuffle=True)), collated on the GPU (pyg_lite.GraphLoader), or on the host and copied
        (pyg_lite.DataLoader) with --host-loader; both draw their permutations from a generator seeded 12345.
        The default 0 keeps the single unshuffled batch.
    python examples/molecule_gcn_train.py --model gat [--layer-count 2]
        --model gat = the SGRACE demo's graph classifier of attention layers (sgrace.GAT_POOL_PYNQ: sym_norm2, two
        GATConv_SGRACE layers with the edge softmax, mean pool, head; fp32 layer buffers), trained layer by layer through
        FPYNQ_GAT's autograd; --layer-count 2 = the accuracy passes run the whole model in one call
        (sgx_gat_stack_forward).  It prints accuracy only: the reference records no GAT output (parity unpinned).
    python examples/molecule_gcn_train.py --model gat --layer-count 2 --qbits 8
        --qbits N (8, 4, 2 or 1; with --model gat) = the layers run the quantised arithmetic of the SGRACE bitstream
        (config.fake_quantization, fp32 emulation of the grid); with --layer-count 2 the accuracy passes are one call of
        sgx_quant_stack_forward.  Parity unpinned here too: the reference records no quantised output.
    python examples/molecule_gcn_train.py --model gat --layer-count 2 --train-stack
        --train-stack = each training step's two attention layers and the pooling run as one forward call
        (sgx_gat_stack_forward) and one backward call (sgx_gat_stack_backward) -- GAT_POOL_PYNQ(train_stack=True); with
        --qbits N the two calls are sgx_quant_stack_forward and sgx_quant_stack_backward
    python examples/molecule_gcn_train.py --model gat --batch-size 64 --layer-count 2 --train-stack [--qbits 8] [--plain-loader]
        --model gat with --batch-size N on the device loader = the shuffled batches arrive ready for the attention layers
        (pyg_lite.GraphLoader(prepare="sym_norm2", quant=sgrace.quant_constants under --qbits): the normalised adjacency,
        its quantised forms and their dead-row facts gathered by the collation launch from what was built once for the
        set), so a step synchronises nowhere; --plain-loader keeps the batches without them (the model then normalises,
        quantises and reads the dead-row flag back per batch), for comparison
    python examples/molecule_gcn_train.py --layer-count 2 --train-stack --trainer [--replay] [--model gat [--qbits 8]]
        --trainer = the tail of every step on the kernels too (train.StackTrainer): dropout, the head, the loss and their
        gradients as one call (sgx_head_loss), Adam over every parameter as one launch (sgx_adam_step), both on a device
        step counter; the dropout stream is the trainer's counter-based mask, not torch's generator.  --replay with
        --batch-size 0 (the single fixed batch) records the whole step once and replays it every epoch.
    python examples/molecule_gcn_train.py --batch-size 64 --layer-count 2 --train-stack --trainer --replay [--model gat]
        --replay on the shuffled batches of the device loader: every full batch arrives padded to one fixed capacity
        (pyg_lite.GraphLoader(pad=True)), and one recorded step -- collation, plan table, forward, loss head, backward,
        Adam -- serves every batch of every epoch (StackTrainer.capture_loader); the short last batch runs eagerly.
        With --trainer the accuracies are counted on the device (StackTrainer.evaluate) and read back in one transfer per
        epoch; with --replay --batch-size N the evaluation replays as well (StackTrainer.capture_eval_loader over
        unshuffled padded loaders of the train and test sets).  With --model gat --qbits 8 the padded batches carry the
        quantised adjacencies (GraphLoader(quant=, pad=True, pad_quant=True)) and the quantised step and passes replay.
        Without --trainer nothing changes
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sgracex1_amd import molecule_gcn as M, pyg_lite as G, pynq_shim  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--acc", type=int, default=1)
    ap.add_argument("--layer-count", type=int, default=1)
    ap.add_argument("--train-stack", action="store_true")
    ap.add_argument("--batch-size", type=int, default=0)
    ap.add_argument("--host-loader", action="store_true")
    ap.add_argument("--plain-loader", action="store_true")
    ap.add_argument("--model", choices=["gcn", "gat"], default="gcn")
    ap.add_argument("--qbits", type=int, default=32, choices=[32, 8, 4, 2, 1])
    ap.add_argument("--trainer", action="store_true")
    ap.add_argument("--replay", action="store_true")
    args = ap.parse_args()
    if args.qbits != 32 and args.model != "gat":
        ap.error("--qbits runs the quantised layers of the SGRACE library: --model gat")
    if args.model == "gat" and args.acc != 1:
        ap.error("--model gat trains on the kernels (--acc 1)")
    if args.train_stack and args.layer_count < 2:
        ap.error("--train-stack needs --layer-count >= 2")
    if args.trainer and not (args.train_stack and args.acc == 1):
        ap.error("--trainer runs the fused training route: --acc 1 --layer-count 2 --train-stack")
    if args.replay and not args.trainer:
        ap.error("--replay replays the trainer's step: --trainer")
    if args.replay and args.batch_size > 0 and (args.host_loader or args.plain_loader):
        ap.error("--replay with --batch-size > 0 takes the device loader's prepared batches")
    if args.host_loader and args.batch_size <= 0:
        ap.error("--host-loader needs --batch-size > 0")
    dev = torch.device("cuda")
    raw = np.load(os.path.join(ROOT, "tests", "golden", "mutag_raw.npz"))
    graphs = G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])
    torch.manual_seed(12345)                                  # MOL cell 6
    graphs = [graphs[i] for i in torch.randperm(len(graphs)).tolist()]
    train, test = G.collate(graphs[:2000]).to(dev), G.collate(graphs[50:100]).to(dev)
    loader = [train]
    if args.batch_size > 0:
        gen = torch.Generator().manual_seed(12345)
        loader = (G.DataLoader(graphs[:2000], batch_size=args.batch_size, shuffle=True, generator=gen) if args.host_loader
                  else G.GraphLoader(graphs[:2000], batch_size=args.batch_size, shuffle=True, generator=gen, device=dev,
                                       pad=args.replay))
    if args.model == "gat":
        from sgracex1_amd import config, sgrace
        config.acc, config.compute_attention = 1, 1
        config.fake_quantization, config.w_qbits = int(args.qbits != 32), args.qbits
        my_ip = sgrace.init_SGRACE()
        my_ip.register_map.layer_count = args.layer_count
        torch.manual_seed(12345)
        gat = sgrace.GAT_POOL_PYNQ(7, 64, 2, train_stack=args.train_stack).to(dev)   # demo_sgrace.py:137-190
        if args.batch_size > 0 and not args.host_loader and not args.plain_loader:
            # the batches layer-ready: normalised (and quantised) once per set, gathered per batch by the collation launch;
            # with --replay padded, the quantised adjacencies with them (pad_quant)
            quantised = dict(quant=sgrace.quant_constants, pad_quant=args.replay and sgrace.quant_constants is not None)
            loader = G.GraphLoader(loader.graphs, batch_size=args.batch_size, shuffle=True, generator=gen, device=dev,
                                   dtypes=(sgrace._torch_dtype(),), prepare="sym_norm2", pad=args.replay, **quantised)
        model = lambda _acc, x, edge_index, batch: gat(x, edge_index, batch)
        model.train, model.eval, model.parameters = gat.train, gat.eval, gat.parameters
    else:
        my_ip = pynq_shim.Overlay("gnn_all.bit").mmult_top_0      # MOL cell 11
        my_ip.register_map.layer_count = args.layer_count          # layers per call (SG.py:1862)
        model = M.GCN_PYNQ(64, 7, 2, my_ip, train_stack=args.train_stack).to(dev)   # MOL cell 18 (seed 12345 inside)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)       # MOL cell 20
    crit = torch.nn.CrossEntropyLoss()
    trainer = replay = replay_epoch = None
    if args.trainer:
        from sgracex1_amd.train import StackTrainer
        trainer = StackTrainer(gat if args.model == "gat" else model, lr=0.01)      # the same Adam, the state on the device
        if args.replay and args.batch_size > 0:
            model.train()
            replay_epoch = trainer.capture_loader(loader)      # one recorded step for every padded batch
        elif args.replay:
            model.train()
            replay = trainer.capture(train.x, train.edge_index, train.batch, train.y)

    eval_passes = None
    if replay_epoch is not None:
        # the accuracy pass replayed too: one recorded evaluation per set over unshuffled padded loaders
        prepared = dict(dtypes=loader.dtypes, prepare=loader.prepare, **quantised) if args.model == "gat" else {}
        eval_passes = [trainer.capture_eval_loader(G.GraphLoader(gs, batch_size=args.batch_size, shuffle=False, device=dev,
                                                                 pad=True, **prepared))
                       for gs in (loader.graphs, graphs[50:100])]

    def accuracy(batch):
        model.eval()
        with torch.no_grad():
            pred = model(args.acc, batch.x, batch.edge_index, batch.batch).argmax(dim=1)
        return float((pred == batch.y).float().mean())

    def accuracies():
        """(train, test) accuracy.  With --trainer the hits are counted on the device (StackTrainer.evaluate, or the
        replayed passes) and both sets' counts come back in ONE transfer; the quotient is the float32 one of accuracy()."""
        if trainer is None:
            return accuracy(train), accuracy(test)
        from sgracex1_amd.train import EvalSums
        if eval_passes is not None:
            for run_pass in eval_passes:
                run_pass()
            sums = [run_pass.sums for run_pass in eval_passes]
        else:
            sums = [EvalSums(dev), EvalSums(dev)]
            for b, into in zip((train, test), sums):
                trainer.evaluate(b.x, b.edge_index, b.batch, b.y, into=into)
        return [float(np.float32(hits) / np.float32(n)) for n, hits, _ in EvalSums.read(*sums)]

    best, log = 0.0, []
    for epoch in range(1, args.epochs + 1):
        model.train()
        t0 = time.perf_counter()
        steps = 0
        if replay_epoch is not None:
            losses = replay_epoch()
            loss, steps = losses[-1], len(losses)
        else:
            for b in loader:
                if args.host_loader:
                    b = b.to(dev)
                if replay is not None:
                    loss = replay()
                elif trainer is not None:
                    loss = trainer.step(b.x, b.edge_index, b.batch, b.y, getattr(b, "num_real_graphs", None))
                else:
                    opt.zero_grad()
                    loss = crit(model(args.acc, b.x, b.edge_index, b.batch), b.y)
                    loss.backward()
                    opt.step()
                steps += 1
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        tr, te = accuracies()
        best = max(best, te)
        log.append({"epoch": epoch, "loss": round(float(loss.detach()), 4), "train_acc": round(tr, 4),
                    "test_acc": round(te, 4), "step_ms": round(dt * 1e3, 3)})
        print(f"Epoch: {epoch:03d}, Train Acc: {tr:.4f}, Test Acc: {te:.4f}, loss {float(loss.detach()):.4f}, "
              f"step {dt * 1e3:.2f} ms", flush=True)
    print(json.dumps({"best_test_acc": best, "final_test_acc": log[-1]["test_acc"], "epochs": args.epochs,
                      "acc": args.acc, "model": args.model, "qbits": args.qbits, "layer_count": args.layer_count, "train_stack": args.train_stack,
                      "batch_size": args.batch_size, "host_loader": args.host_loader,
                      **({"trainer": True, "replay": args.replay} if args.trainer else {}),
                      "prepared_loader": bool(getattr(loader, "prepare", None)), "reference": "0.76 at epoch 34 (notebook cell 20 output)" if args.model == "gcn" else "none (parity unpinned)"}))


if __name__ == "__main__":
    main()
