"""The few torch_geometric pieces the reference's notebooks use around the hot path, restated
with plain torch so the end-to-end runs do not need PyG (it is not installed here): the TU
dataset reader for MUTAG (raw files -> graphs), DataLoader-style batching into one block-
diagonal graph, `to_dense_adj`, `global_mean_pool` (MOL cells 4-10, 18), the same shuffled batches collated on the GPU
(GraphLoader), and the NeighborLoader of the node-classification demo's mini-batch mode (demo_sgrace.py:112-125),
sampled on the GPU.
"""
import weakref
from dataclasses import dataclass
from typing import List

import numpy as np
import torch


@dataclass
class Graph:
    x: torch.Tensor            # [n, F] one-hot node labels
    edge_index: torch.Tensor   # [2, E] int64
    y: torch.Tensor            # [1] int64

    @property
    def num_nodes(self):
        return self.x.shape[0]


@dataclass
class Batch:
    x: torch.Tensor
    edge_index: torch.Tensor
    y: torch.Tensor
    batch: torch.Tensor        # [n] graph id of every node
    num_graphs: int
    num_real_graphs: int = None    # a padded batch (GraphLoader(pad=True)): its first graphs are the real ones; else all

    def __post_init__(self):
        if self.num_real_graphs is None:
            self.num_real_graphs = self.num_graphs

    @property
    def num_nodes(self):
        return self.x.shape[0]

    def to(self, device):
        return Batch(self.x.to(device), self.edge_index.to(device), self.y.to(device), self.batch.to(device),
                     self.num_graphs, self.num_real_graphs)


def load_tu_raw(A, graph_indicator, graph_labels, node_labels) -> List[Graph]:
    """TU format (MUTAG/raw/*.txt): A = 1-based (row, col) pairs, graph_indicator = 1-based graph
    id per node, labels {-1, 1} -> {0, 1} as torch_geometric's TUDataset does, node labels one-hot."""
    A = np.asarray(A, np.int64) - 1
    gi = np.asarray(graph_indicator, np.int64) - 1
    nl = np.asarray(node_labels, np.int64)
    labels = np.asarray(graph_labels, np.int64)
    uniq = np.unique(labels)
    y = np.searchsorted(uniq, labels)
    n_feat = int(nl.max()) + 1
    n_graphs = int(gi.max()) + 1
    first = np.searchsorted(gi, np.arange(n_graphs))
    count = np.bincount(gi, minlength=n_graphs)
    edge_graph = gi[A[:, 0]]
    graphs = []
    for g in range(n_graphs):
        e = A[edge_graph == g] - first[g]
        x = torch.zeros((count[g], n_feat))
        x[torch.arange(count[g]), torch.as_tensor(nl[first[g]:first[g] + count[g]])] = 1.0
        graphs.append(Graph(x, torch.as_tensor(e.T.copy()), torch.tensor([y[g]])))
    return graphs


def collate(graphs: List[Graph]) -> Batch:
    xs, es, ys, bs = [], [], [], []
    off = 0
    for i, g in enumerate(graphs):
        xs.append(g.x)
        es.append(g.edge_index + off)
        ys.append(g.y)
        bs.append(torch.full((g.num_nodes,), i, dtype=torch.int64))
        off += g.num_nodes
    return Batch(torch.cat(xs), torch.cat(es, dim=1), torch.cat(ys), torch.cat(bs), len(graphs))


class DataLoader:
    def __init__(self, dataset, batch_size=1, shuffle=False, generator=None):
        self.dataset, self.batch_size, self.shuffle, self.generator = list(dataset), batch_size, shuffle, generator

    def __iter__(self):
        n = len(self.dataset)
        order = torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))
        for i in range(0, n, self.batch_size):
            yield collate([self.dataset[j] for j in order[i:i + self.batch_size]])

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size


class GraphLoader:
    """DataLoader(dataset, batch_size, shuffle, generator) with the dataset on the GPU (ops.GraphSet, uploaded once) and
    every batch collated there by one kernel launch (ops.collate_graphs): the same permutation rule as DataLoader --
    torch.randperm(n, generator=generator) on the host, contiguous slices, a partial last batch kept -- and the same
    Batch contents, as device tensors.  Each batch arrives with what the fused GCN stack needs already attached, so
    GCN_PYNQ runs it without a device synchronisation: graph_ptr on `batch` (ops.graph_ptr_of), the adjacency on
    `edge_index` ("adj_csr", n, dtype) and the feature CSR on `x` ("fea_csr", dtype) for each of `dtypes`, and on
    graph_ptr the block facts (its largest graph) from which ops.BatchPlan.cached builds trusted plans.
    dataset: a list of Graph, or an ops.GraphSet.

    prepare="sym_norm2": every batch also arrives ready for sgrace.GAT_POOL_PYNQ, whose forward then computes nothing
    before its first kernel and reads nothing back.  The normalised adjacency of the whole set is built once
    (ops.GraphSet.prepare_sym_norm2; rule in include/sgx.h) and the same collation launch gathers each batch's rows of it:
    edge_index carries what the model looks up -- ("sym_norm2", n, 1, dtype) -> (edge_index, values, normalised Csr) for
    each of `dtypes`, the Csr with its dead-row mask, flag and longest row recorded -- and graph_ptr's block facts name
    that Csr's column array, so that the batch plans of the fused stack are the trusted ones.  The kernels read the Csr;
    the list of the attached triple is edge_index itself (the stored edges without the added loops).
    quant=qc (a quant.QuantConstants such as sgrace.quant_constants; with prepare, and float32 among dtypes): the float32
    Csr also holds .quantized(qc) and .quantized(qc.second_layer()) with their dead-row facts, gathered from values
    quantised once per set.  prepare=None: the batches as before.

    pad=True: the same permutation rule and the same batches, and every batch that fits -- exactly batch_size graphs, at
    most pad_rows rows (default: the batch_size largest graphs' rows, so every full batch fits) -- arrives PADDED to one
    fixed capacity (ops.pad_capacity; rule in include/sgx.h, "padded batches"): every tensor has the same size in every
    batch, the batch's graphs come first (Batch.num_real_graphs of them) and filler graphs behind -- rows whose x is 0
    and whose adjacency row is one diagonal 1, labels 0 -- which pool to 0 and receive no gradient.  A loss takes
    out[:batch.num_real_graphs] and y[:batch.num_real_graphs]; past the stored edges edge_index holds -1: it is the key
    of the attached CSRs, which the kernels read, not an edge list.  One recorded training step then serves every such
    batch (train.StackTrainer.capture_loader).  A short last batch, a batch over pad_rows and, from a prepared loader, a
    batch with a dead-row graph (a host fact of the prepared set: the fused attention route declines such a batch, and
    the layer-by-layer route it then takes was written for CSRs without spare capacity) arrive unpadded, as before.  A
    padded batch is made for the fused stack routes, which read the attached CSRs through their row pointers;
    train.StackTrainer.step refuses to run one layer by layer, and the attention model takes padded batches from a
    prepare="sym_norm2" loader only (it would otherwise normalise the padded edge_index).

    pad=True with quant= takes pad_quant=True as well (ValueError without it): the padded batches then carry the quantised
    adjacencies of both layers at capacity size (ops.collate_graphs(pad_quant=True), sgx_collate_graphs_padded_quant) -- a
    filler row's diagonal entry holds the grid's image of 1, the spare entries its image of 0, the Csrs' facts say "no
    dead row" and carry the set's longest row, as an unpadded prepared batch's -- so the fused quantised stack
    (ops.QuantStack) runs them and one recorded step serves every such batch.  The constants must keep a filler graph
    inert, which is checked here on the host before any device work (ValueError naming quant): on the adjacency grid of
    quant and quant.second_layer() 1 stays positive and 0 stays 0 (check_pad_quant), and on their feature grids 0 stays 0
    (a filler row's zero output is the next layer's input).  A batch with a graph that has a dead row under the
    quantised mask of either layer (a host fact of the prepared set; at 4 bits and below an entry may round to 0) arrives
    unpadded, like a batch with a dead-row graph."""

    def __init__(self, dataset, batch_size=1, shuffle=False, generator=None, device=None, dtypes=(torch.float16,),
                 prepare=None, quant=None, pad=False, pad_rows=None, pad_quant=False):
        from . import ops
        if pad_quant and not (pad and quant is not None):
            raise ValueError("pad_quant=True needs pad=True and quant=: it pads the quantised adjacencies of a padding loader")
        if pad and quant is not None and not pad_quant:
            raise ValueError("pad=True with quant= needs pad_quant=True: without it padded batches do not carry the quantised "
                             "adjacencies")
        if pad_quant:
            check_pad_quant(quant)
            check_pad_quant_features(quant)
        if pad_rows is not None and not pad:
            raise ValueError("pad_rows needs pad=True")
        if quant is not None and not prepare:
            raise ValueError("quant needs prepare='sym_norm2'")
        if prepare not in (None, "sym_norm2"):
            raise ValueError(f"prepare must be None or 'sym_norm2', not {prepare!r}")
        if quant is not None and torch.float32 not in tuple(dtypes):
            raise ValueError("quant needs dtype=torch.float32: the quantised layer works on float32 buffers")
        self.graphs = dataset if isinstance(dataset, ops.GraphSet) else ops.GraphSet(dataset, device or "cuda")
        self.batch_size, self.shuffle, self.generator = int(batch_size), bool(shuffle), generator
        self.dtypes = tuple(dtypes)
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.prepare, self.quant = prepare, quant
        self.extras = self.graphs.prepare_sym_norm2(self.dtypes, quant) if prepare else None
        self.pad, self.pad_quant = bool(pad), bool(pad_quant)
        # (after the set is prepared: the capacity counts the normalised adjacency's entries too)
        self.capacity = ops.pad_capacity(self.graphs, min(self.batch_size, len(self.graphs)), pad_rows) if self.pad else None

    def __len__(self):
        return (len(self.graphs) + self.batch_size - 1) // self.batch_size

    def batches(self):
        """The graph ids of the next epoch's batches (host arrays, in order): one draw from the generator, as an epoch of
        __iter__ takes."""
        n = len(self.graphs)
        order = torch.randperm(n, generator=self.generator).numpy() if self.shuffle else np.arange(n)
        return [order[i:i + self.batch_size] for i in range(0, n, self.batch_size)]

    def __iter__(self):
        for ids in self.batches():
            yield self.collate(ids)

    def padded(self, idx):
        """Whether the batch of graph ids `idx` arrives padded: pad=True, exactly batch_size graphs, rows within the
        capacity and, with a prepared adjacency, no graph with a dead row -- under the normalised values or, with
        pad_quant, under the quantised values of either layer.  Host only."""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if not self.pad or not self.capacity.fits(idx.size, int(self.graphs.counts[0][idx].sum())):
            return False
        return self.extras is None or not bool(self.has_dead()[idx].any())

    def has_dead(self):
        """Per graph of a prepared set (host bool [graphs]): it has a dead row under the normalised adjacency or, from a
        loader with pad_quant, under the quantised adjacency of either layer -- the graphs whose batches arrive unpadded."""
        p = self.extras.prepared
        dead = p.has_dead
        for key in (self.extras.keys if getattr(self, "pad_quant", False) else ()):
            dead = dead | p.quant[key][2]
        return dead

    def collate(self, idx, out=None):
        """The Batch of graph ids `idx` (host, in batch order, or an ops.BatchIndex of them), caches attached; out: an
        ops.Collated to reuse."""
        from . import ops
        ids = idx.ids if isinstance(idx, ops.BatchIndex) else idx
        padded = self.padded(ids)
        c = ops.collate_graphs(self.graphs, idx, self.dtypes, out=out, extras=self.extras,
                               pad=self.capacity if padded else None, pad_quant=padded and self.pad_quant)
        return attach_batch(c)


def attach_batch(c):
    """A pyg_lite.Batch over the tensors of an ops.Collated, with its graph_ptr, CSRs and block facts attached -- and,
    where it was collated with extras, the normalised adjacency with its facts and quantised forms."""
    from . import ops
    n, B = c.x.shape[0], c.index.n_graphs
    G, max_graph = (B, c.index.max_graph) if c.pad is None else (c.pad.n_graphs, c.pad.filler_rows)
    ops.attach(c.batch, ("graph_ptr",), c.graph_ptr)
    cols = []
    if c.extras is not None:
        p, ids = c.extras.prepared, c.index.ids
        for dt in c.extras.dtypes:
            N = ops.Csr(c.norm_rowptr, c.norm_col, c.norm_val[dt], n).with_facts(c.norm_dead, p.has_dead[ids].any(), p.max_row)
            if dt == torch.float32:
                for key in c.extras.keys:
                    N._quantized[key] = ops.Csr(N.rowptr, N.col, c.q_val[key], n).with_facts(
                        c.q_dead[key], p.quant[key][2][ids].any(), p.max_row)
            ops.attach(c.edge_index, ("sym_norm2", n, 1, dt), (c.edge_index, N.val, N))
        cols.append(weakref.ref(c.norm_col))
    for dt, val in c.adj_val.items():
        A = ops.Csr(c.adj_rowptr, c.adj_col, val, n)
        cols.append(weakref.ref(A.col))            # (weak: the adjacency's cache already holds graph_ptr)
        ops.attach(c.edge_index, ("adj_csr", n, dt), A)
        ops.attach(c.x, ("fea_csr", dt), ops.Csr(c.fea_rowptr, c.fea_col, c.fea_val[dt], c.n_feat))
    ops.attach(c.graph_ptr, ("block_facts",), {"n_rows": n, "max_graph": max_graph, "cols": cols, "padded": c.pad is not None})
    return Batch(c.x, c.edge_index, c.y, c.batch, G, B)


def to_dense_adj(edge_index, num_nodes=None):
    """[1, N, N] 0/1 adjacency (duplicates add up, as torch_geometric.utils.to_dense_adj)."""
    n = int(edge_index.max()) + 1 if num_nodes is None else num_nodes
    adj = torch.zeros((n, n), dtype=torch.float32, device=edge_index.device)
    adj.index_put_((edge_index[0], edge_index[1]), torch.ones(edge_index.shape[1], device=edge_index.device),
                   accumulate=True)
    return adj.unsqueeze(0)


def global_mean_pool(x, batch, size=None):
    size = int(batch.max()) + 1 if size is None else size
    out = torch.zeros((size, x.shape[1]), dtype=x.dtype, device=x.device)
    out.index_add_(0, batch, x)
    cnt = torch.bincount(batch, minlength=size).clamp(min=1).to(x.dtype)
    return out / cnt.unsqueeze(1)


def add_remaining_self_loops(edge_index, edge_weight, fill_value, num_nodes):
    """Self loop (weight fill_value) for every node that has none; existing loops keep their weight."""
    row, col = edge_index
    has = torch.zeros(num_nodes, dtype=torch.bool, device=row.device)
    has[row[row == col]] = True
    missing = torch.nonzero(~has).reshape(-1)
    ei = torch.cat([edge_index, torch.stack([missing, missing])], dim=1)
    ew = torch.cat([edge_weight, torch.full((missing.numel(),), float(fill_value), dtype=edge_weight.dtype,
                                            device=row.device)])
    return ei, ew


def sort_edge_index(edge_index, edge_weight, num_nodes):
    key = edge_index[0] * num_nodes + edge_index[1]
    perm = torch.argsort(key, stable=True)
    return edge_index[:, perm], edge_weight[perm]


class NodeData:
    """A node-classification graph as the demo's Planetoid / Amazon datasets carry it: x, y, edge_index and optional
    train / val / test masks."""

    def __init__(self, x, edge_index, y=None, train_mask=None, val_mask=None, test_mask=None):
        self.x, self.edge_index, self.y = x, edge_index, y
        self.train_mask, self.val_mask, self.test_mask = train_mask, val_mask, test_mask

    @property
    def num_nodes(self):
        return self.x.shape[0]


class NodeBatch:
    """One NeighborLoader batch, PyG's surface: x / y / masks / n_id of the sampled nodes (seeds first), edge_index in
    local ids oriented as PyG does (row 0 = sampled neighbour, row 1 = the node it was sampled for), batch_size,
    input_id (positions of the seeds in input_nodes), num_sampled_nodes / num_sampled_edges per hop; plus adj, the same
    edges as a Csr whose row i holds the neighbours sampled for local node i (aggregation at the seed rows).
    From a loader with prepare="sym_norm2" also edge_index_agg (edge_index with its rows swapped: row 0 the aggregating
    node, what the SGRACE layers take) and adj_norm (the Csr of sym_norm2 over it).
    num_real_nodes: the sampled nodes' count -- None for a padded batch (NeighborLoader(pad=True)), whose tensors have the
    capacity's sizes (filler rows behind the live ones: n_id = -1, x = 0, y = 0, masks False) and whose live count stays on
    the device, in loader.counts; adj, num_sampled_nodes and num_sampled_edges are None there as well."""

    num_real_nodes = None

    def __init__(self, **fields):
        self.__dict__.update(fields)

    @property
    def num_nodes(self):
        return self.n_id.numel()


_MASKS = ("train_mask", "val_mask", "test_mask")


def _fq_unsigned_scalar(x, s, z, qbits):
    """sgrace._fq_unsigned (quantization_ufbits, SG.py:253-265) of one number, on the host, as the library evaluates it:
    1 / s rounded to fp32 (what ops hands the C ABI as inv_scale_adj), the product and the sum each rounded to fp32, round
    half to even, the clip and the division."""
    import numpy as np
    f = np.float32
    t = f(f(1.0 / s) * f(x)) + f(z)
    q = min(max(float(np.rint(f(t))), 0.0), float(2 ** qbits - 1))
    return q / 2 if qbits == 1 else q / 2 ** (qbits - 1)


def check_pad_quant(quant):
    """The conditions NeighborLoader(pad=True, quant=) puts on the adjacency's quantiser constants (include/sgx.h, "padded
    node batches"), for `quant` and quant.second_layer(): ValueError naming `quant` where one fails.  Host arithmetic only."""
    import math
    try:
        sets = [(int(qc.w_qbits), float(qc.a_s), float(qc.a_z)) for qc in (quant, quant.second_layer())]
    except (AttributeError, TypeError, ValueError) as e:
        raise ValueError(f"pad=True with quant=: quant carries no adjacency constants (w_qbits, a_s, a_z): {e}") from None
    for bits, a_s, a_z in sets:
        if bits not in (8, 4, 2, 1):
            raise ValueError(f"pad=True with quant=: quant.w_qbits must be 8, 4, 2 or 1, not {bits}")
        if not (math.isfinite(a_s) and a_s > 0 and math.isfinite(a_z)):
            raise ValueError(f"pad=True with quant=: quant.a_s must be finite and positive (a_s {a_s}, a_z {a_z})")
        one, zero = _fq_unsigned_scalar(1.0, a_s, a_z, bits), _fq_unsigned_scalar(0.0, a_s, a_z, bits)
        if not one > 0:
            raise ValueError(f"pad=True with quant=: with quant's a_s {a_s}, a_z {a_z} at {bits} bits a filler row's diagonal 1 "
                             "rounds to 0: the filler rows would be dead under the quantised mask")
        if zero != 0:
            raise ValueError(f"pad=True with quant=: with quant's a_s {a_s}, a_z {a_z} at {bits} bits a filler row's spare 0 "
                             f"becomes {zero}: the spare entries would carry weight")


def check_pad_quant_features(quant):
    """What GraphLoader(pad_quant=True) asks of the FEATURE grids of `quant` and quant.second_layer() besides
    check_pad_quant (include/sgx.h, "padded batches ready for the quantised layers"): 0 stays 0, so that a filler row's
    zero output is a zero input of the next quantised layer.  ValueError naming `quant` otherwise.  Host arithmetic only."""
    import math
    for qc in (quant, quant.second_layer()):
        bits, f_s, f_z = int(qc.w_qbits), float(qc.f_s), float(qc.f_z)
        if not (math.isfinite(f_s) and f_s > 0 and math.isfinite(f_z)):
            raise ValueError(f"pad_quant=True: quant.f_s must be finite and positive (f_s {f_s}, f_z {f_z})")
        zero = _fq_unsigned_scalar(0.0, f_s, f_z, bits)
        if zero != 0:
            raise ValueError(f"pad_quant=True: with quant's f_s {f_s}, f_z {f_z} at {bits} bits a filler row's zero output "
                             f"becomes {zero} as the next layer's input: the filler graphs would not stay inert")


class NeighborLoader:
    """torch_geometric.loader.NeighborLoader(data, num_neighbors, batch_size, input_nodes, shuffle) on the HIP sampler
    (ops.sample_neighbors, rule in include/sgx.h).  The CSR on the targets of edge_index (row v = the edges j -> v,
    flow="source_to_target", repeated edges kept) is built once per loader.  An epoch visits every input node once, in
    order or in a permutation drawn from `seed` and the epoch number; batch b of epoch e samples with step
    e * len(loader) + b, so every batch is reproducible.

    prepare="sym_norm2" (with `fill` and `dtype`, the layer's element type): every batch arrives layer-ready, built on the
    GPU right behind the sample inside the sampler's single synchronisation (ops.sample_node_batch): edge_index_agg
    carries what GAT_PYNQ.forward looks up -- ("sym_norm2", n, 1, dtype) -> (edge list, values, normalised Csr with its
    dead-row mask, flag and longest row) -- and x carries ("fea_csr", dtype), gathered from the CSR of data.x built once
    here.  Pass batch.edge_index_agg to the model; it then computes nothing before its first kernel.  The list of the
    attached triple is edge_index_agg itself (the sampled edges without the added loops); the kernels read the Csr.
    The seeds are rows 0 .. batch_size-1, so a loss over them is out[:batch.batch_size].  prepare=None: the batches as
    before.

    transposed=True (with prepare): every batch also carries what the backward would otherwise build per batch from a
    sort -- x the fp32 feature CSR under ("fea_csr", float32) and its transpose under ("fea_csr_t", float32), the two
    entries ops.feature_csr32 looks up (config.accb = 1 over CSR features), and adj_norm._transpose_pattern = (A^T,
    order), what the default GAT backward looks up -- from two sgx_csr_transpose calls on the same stream behind the
    sampler, with no synchronisation of their own (a transposed matrix that wants a plan by ops.csr_transpose's rule
    still builds it, with the plan's read-back).

    quant=qc (a quant.QuantConstants such as sgrace.quant_constants; with prepare and dtype float32): the batches are ready
    for the QUANTISED layers as well -- adj_norm.quantized(qc) and .quantized(qc.second_layer()), what the layers look up,
    are delivered with their dead-row facts and the lean GAT backward's mask values, from the sampler's own launches and
    single read-back (ops.sample_node_batch(quant=)).  A training step of the quantised model then synchronises nowhere
    outside the sampler.

    pad=True (with prepare="sym_norm2"): the same batches, and every FULL batch (exactly batch_size seeds) arrives PADDED to
    one fixed capacity (ops.node_pad_capacity; rule in include/sgx.h, "padded node batches"): every tensor has the same
    size in every batch, the sampled nodes come first and filler rows behind them -- x 0, n_id -1, y 0, masks False, an
    adjacency row of one diagonal 1 -- which yield 0 in every layer and receive no gradient from a loss over the seeds,
    out[:batch.batch_size].  Nothing is read back: no synchronisation, batch.num_real_nodes is None and the live counts
    stay on the device (loader.counts, int32: nodes, edges, adjacency entries, feature entries, then per hop); the facts
    the layers ask for are constants (longest row max(max(fanouts) + 1, 64), has_dead_rows = True with the exact mask).  A
    padded batch lives in ONE set of buffers that the next batch overwrites: it is valid until the next one is drawn.
    One recorded training step then serves every full batch (train.NodeTrainer.capture_loader).  The short last batch
    arrives unpadded, as before.  What the eager call raises for a batch (repeated seeds) is OR-ed into a device word
    instead; loader.status() reads it back once -- at the end of an epoch, say -- and raises it then.  transposed=True
    works as before for the adjacency; the feature transpose is delivered only where it wants no plan (fewer than 64
    entries per feature column at capacity), since a plan costs a read-back -- config.accb = 1 is a padded route only
    with schedule="flat" (below).
    With attention on, a live row without a positive entry (fill = 0 leaves the rows of the last hop so) takes its
    uniform softmax over the N padded columns rather than the live ones: the layers' rule, on the padded width.
    ValueError where a batch CSR would want a plan (ops.Csr.wants_plan), which costs a read-back: a fan-out of -1,
    max(fanouts) + 1 > 64, a feature row of over 64 entries, 2^20 or more adjacency or feature entries.

    pad=True with quant=qc: the padded batches carry the quantised adjacencies too, at capacity size and with the same
    constant facts (ops.sample_node_batch(pad=, quant=), sgx_node_batch_sample_padded_quant): a filler row holds fq(1) on
    its diagonal entry and fq(0) on its spare ones, fq the unsigned-grid quantiser of the adjacency.  The constants are
    checked here, before any device work (check_pad_quant): w_qbits in {8, 4, 2, 1}, a finite positive a_s, fq(1) > 0 -- no
    filler row is dead under the quantised mask -- and fq(0) == 0 -- its spare entries carry no weight; ValueError naming
    `quant` otherwise.  quant.constants(w) passes at every width.  The recorded step then covers the quantised model as
    well; the short last batch takes the unpadded quant= route.

    schedule="flat" (with pad=True; None by default): the batches are for the entry-split schedule -- adj_norm, the feature
    CSR and, with transposed=True, the transposed pattern and X^T (always delivered) arrive with_facts(flat=True) at their
    honest longest row, so none of them wants a plan (ops.Csr.wants_plan), at capacity and for the short last batch alike,
    and the layers take sgx_layer_forward's SGX_SCHEDULE_FLAT, ops.spmm / ops.gat_aggregate(schedule="flat") for them.
    config.accb = 1 takes them too (with transposed=True): sgx_layer_backward runs the adjacency's products, Wh = X . W and
    X^T . pg on its entry-split schedules at the capacities, so the one-call backward records and replays as well.
    The three refusals that exist because a plan costs a read-back then do not apply: max(fanouts) + 1 > 64, feature
    rows of over 64 entries, capacities from 2^20 entries.  Still refused: a fan-out of -1 (an unbounded row has no
    capacity) and quant= (the quantised layer has no entry-split epilogue yet) -- unless flat_quant=True is passed as well.

    flat_quant=True (with pad=True, schedule="flat" and quant=qc; ValueError without them): the quantised layers' opt-in to
    the entry-split schedule.  The batches come from the padded quantised sampler as under pad=True with quant= (the same
    host checks on qc: fq(1) > 0, fq(0) == 0), and every CSR -- adj_norm, both layers' quantised adjacencies with the lean
    backward's mask values, the feature CSR, the transposes -- arrives with_facts(flat=True, flat_quant=True), the pair of
    facts on which ops.layer_forward(quant=) and sgrace.FPYNQ_GAT (config.accb = 0) take SGX_SCHEDULE_FLAT with
    SGX_QUANT_FLAT.  So the default quantised model records a step at any fan-out.  config.accb = 1 with a quantiser
    keeps the row schedule in its backward and is not a padded route here."""

    def __init__(self, data, num_neighbors, batch_size=1, input_nodes=None, shuffle=False, seed=0, prepare=None, fill=0,
                 dtype=torch.float32, transposed=False, quant=None, pad=False, schedule=None, flat_quant=False):
        from . import ops
        if schedule not in (None, "flat"):
            raise ValueError(f"schedule must be None or 'flat', not {schedule!r}")
        if schedule == "flat" and not pad:
            raise ValueError("schedule='flat' needs pad=True: it is the padded batches' route past the plan refusals")
        if flat_quant and not (schedule == "flat" and quant is not None):
            raise ValueError("flat_quant=True needs schedule='flat' and quant=: it is the quantised layers' opt-in to that schedule")
        if schedule == "flat" and quant is not None and not flat_quant:
            raise ValueError("quant= does not go with schedule='flat': the quantised layer has no entry-split epilogue yet")
        self.schedule, self.flat_quant = schedule, bool(flat_quant)
        flat = schedule == "flat"
        if pad and prepare != "sym_norm2":
            raise ValueError("pad=True needs prepare='sym_norm2'")
        if pad and any(int(k) < 0 for k in num_neighbors):
            raise ValueError("pad=True needs fan-outs >= 0: a fan-out of -1 leaves a row unbounded")
        if pad and not flat and max(int(k) for k in num_neighbors) + 1 > 64:
            raise ValueError("pad=True needs max(num_neighbors) + 1 <= 64: a longer adjacency row wants a plan, and a plan "
                             "costs a read-back")
        if quant is not None and not prepare:
            raise ValueError("quant needs prepare='sym_norm2'")
        if quant is not None and dtype != torch.float32:
            raise ValueError("quant needs dtype=torch.float32: the quantised layer works on float32 buffers")
        if pad and quant is not None:
            check_pad_quant(quant)
        self.quant = quant
        self.data, self.num_neighbors = data, [int(k) for k in num_neighbors]
        self.batch_size, self.shuffle, self.seed = int(batch_size), bool(shuffle), int(seed)
        x, ei = data.x, data.edge_index
        n = x.shape[0]
        dev = x.device
        if input_nodes is None:
            input_nodes = torch.arange(n, device=dev)
        elif input_nodes.dtype == torch.bool:
            input_nodes = torch.nonzero(input_nodes.to(dev)).reshape(-1)
        self.input_nodes = input_nodes.to(dev, torch.int64)
        dst, src = ei[1].to(dev, torch.int64), ei[0].to(dev, torch.int64)
        order = torch.argsort(dst * n + src, stable=True)
        self.csr = ops.Csr.from_coo(dst[order].to(torch.int32), src[order].to(torch.int32),
                                    torch.ones(order.numel(), dtype=torch.float32, device=dev), n, n)
        self.epoch = 0
        if prepare not in (None, "sym_norm2"):
            raise ValueError(f"prepare must be None or 'sym_norm2', not {prepare!r}")
        self.prepare, self.fill, self.dtype = prepare, fill, dtype
        if transposed and not prepare:
            raise ValueError("transposed=True needs prepare='sym_norm2'")
        self.transposed = bool(transposed)
        if prepare:
            ops.dtype_code(dtype)
            if x.dtype != torch.float32 or not x.is_contiguous():
                raise TypeError("a preparing NeighborLoader takes data.x as a contiguous float32 tensor")
            self.fea = ops.feature_csr(x)                           # once per loader; batches gather their rows from it
            self.y = None if getattr(data, "y", None) is None else data.y.to(dev, torch.int64).contiguous()
            self.masks = [(name, getattr(data, name).to(dev, torch.bool).contiguous()) for name in _MASKS
                          if getattr(data, name, None) is not None]
        self.pad = bool(pad)
        if self.pad:
            m = self.input_nodes
            if m.numel() and (int(m.min()) < 0 or int(m.max()) >= n):      # (once per loader; a batch's status is not read)
                raise ValueError("input_nodes must be node ids of the graph")
            if not flat and self.fea._max_row > 64:
                raise ValueError("pad=True needs feature rows of at most 64 entries: a longer one wants a plan, and a plan "
                                 "costs a read-back")
            B = min(self.batch_size, n)
            self.capacity = cap = ops.node_pad_capacity(self.csr, B, self.num_neighbors, self.fea)
            if not flat and (cap.nnz_norm >= 1 << 20 or cap.nnz_fea >= 1 << 20):
                raise ValueError(f"pad=True: the capacity ({cap.nnz_norm} adjacency, {cap.nnz_fea} feature entries) reaches 2^20 "
                                 "entries: such a batch wants a plan, and a plan costs a read-back")
            self.buffers = ops.NodePadBuffers(cap, n, dtype, dev, x.shape[1], self.y is not None, len(self.masks),
                                              len(ops._adj_quant_sets(quant)))
            self.counts = self.buffers.counts
            self.seeds_buf = torch.zeros(B, dtype=torch.int32, device=dev)      # what a recorded sample reads: load()
            self.step_buf = torch.zeros(1, dtype=torch.int64, device=dev)
            self.x_buf = torch.zeros((cap.n_rows, x.shape[1]), dtype=x.dtype, device=dev)

    def __len__(self):
        return (self.input_nodes.numel() + self.batch_size - 1) // self.batch_size

    def epoch_batches(self):
        """(seeds, input_id, step) of the next epoch's batches, in order, as __iter__ samples them; takes one epoch number."""
        m = self.input_nodes.numel()
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed * 1000003 + self.epoch)
            # (pinned and non-blocking: the epoch's one upload does not synchronise)
            perm = torch.randperm(m, generator=g).pin_memory().to(self.input_nodes.device, non_blocking=True)
        else:
            perm = torch.arange(m, device=self.input_nodes.device)
        first_step, self.epoch = self.epoch * len(self), self.epoch + 1
        for b, i in enumerate(range(0, m, self.batch_size)):
            input_id = perm[i:i + self.batch_size]
            yield self.input_nodes[input_id], input_id, first_step + b

    def __iter__(self):
        for seeds, input_id, step in self.epoch_batches():
            yield self._batch(seeds, input_id, step)

    def padded(self, seeds):
        """Whether the batch of `seeds` arrives padded: pad=True and a full batch.  Host only."""
        return self.pad and seeds.numel() == self.capacity.batch_size

    def load(self, seeds, step):
        """The seeds and the step word of the next padded batch, copied into the fixed buffers padded_batch() reads (two
        launches, no synchronisation): what changes between two replays of a recorded padded_batch()."""
        self.seeds_buf.copy_(seeds)
        self.step_buf.fill_(int(step))

    def padded_batch(self, input_id=None):
        """The padded NodeBatch of what load() put in place, drawn into the loader's one set of buffers: every launch of
        it is capturable, and it reads nothing back."""
        s = self._sample(self.seeds_buf, self.step_buf, pad=self.capacity, out=self.buffers)
        return self._hand_over(s, self.x_buf, input_id)


    def status(self):
        """Reads the OR-ed status word of the padded batches drawn since the last call back (one synchronisation), clears
        it, and raises what the eager call would have raised for such a batch (ops.SgxError)."""
        from . import _lib
        st = int(self.buffers.status.item())
        self.buffers.status.zero_()
        if st:
            # (the sampler's status bits as sgx_node_batch_sample maps them: 1 = seeds, else a capacity = SGX_ERR_SHAPE, -2)
            raise _lib.SgxError(_lib.SGX_ERR_SEEDS if st & 1 else -2, "sgx_node_batch_sample_padded")

    def _sample(self, seeds, step, **pad):
        from . import ops
        return ops.sample_node_batch(self.csr, seeds, self.num_neighbors, seed=self.seed, step=step, fill=self.fill,
                                     dtype=self.dtype, features=self.fea, y=self.y, masks=[m for _, m in self.masks],
                                     quant=self.quant, **pad)

    def _prepared(self, seeds, input_id, step):
        """The unpadded layer-ready NodeBatch of `seeds` at `step`: the sampler's one synchronisation."""
        return self._hand_over(self._sample(seeds, step), None, input_id)

    def _hand_over(self, s, x_buf, input_id):
        """The NodeBatch of the NodeSample `s` with everything the layers look up attached: x gathered into x_buf (the
        padded loader's buffer; None: a fresh tensor of an unpadded batch).  Launches only, no synchronisation of its own."""
        from . import ops
        padded = x_buf is not None
        x = ops.pack_rows(self.data.x, s.n_id, out=x_buf)
        A, fea, n = s.adj_norm, s.fea, s.n_id.numel()           # (n: the capacity's rows when padded)
        flat = self.schedule == "flat"
        if flat:                                                # the entry-split schedule: no plan for either, whatever their rows
            fq = self.flat_quant or None                        # ... under the quantiser too, where the loader was asked
            A.with_facts(flat=True, flat_quant=fq)
            fea.with_facts(flat=True, flat_quant=fq)
            if fq:                                              # the layers look these up (Csr.quantized, sgrace._lean_mask)
                for Q in A._quantized.values():
                    Q.with_facts(flat=True, flat_quant=True)
                    if getattr(Q, "_lean_values", None) is not None:
                        Q._lean_values.with_facts(flat=True, flat_quant=True)
        ops.attach(x, ("fea_csr", self.dtype), fea)
        ops.attach(s.edge_index_agg, ("sym_norm2", n, 1, self.dtype), (s.edge_index_agg, A.val[:A.nnz], A))
        if self.transposed:
            # (padded: ops.csr_transpose builds a plan, with its read-back, from 64 entries per feature column on)
            # (the transpose of a flat-marked matrix is flat-marked and builds none)
            if not padded or flat or self.capacity.nnz_fea < 64 * fea.n_cols:
                fea32 = fea
                if self.dtype != torch.float32:          # (the values alone are cast: never through a dense tensor)
                    fea32 = ops.attach(x, ("fea_csr", torch.float32),
                                       ops.Csr(fea.rowptr, fea.col[:fea.nnz], fea.val[:fea.nnz].float(), fea.n_cols).with_facts(
                                           max_row=fea._max_row, flat=fea._flat, flat_quant=fea._flat_quant))
                ops.attach(x, ("fea_csr_t", torch.float32), ops.csr_transpose(fea32, method="device"))
            A._transpose_pattern = ops.csr_transpose(A, return_order=True, method="device")
        fields = dict(x=x, edge_index=s.edge_index, edge_index_agg=s.edge_index_agg, adj_norm=A, n_id=s.n_id.long(),
                      adj=s.adj, batch_size=s.batch_size, input_id=input_id, num_sampled_nodes=s.num_sampled_nodes,
                      num_sampled_edges=s.num_sampled_edges, num_real_nodes=None if padded else n)
        if s.y is not None:
            fields["y"] = s.y
        for (name, _), m in zip(self.masks, s.masks):
            fields[name] = m
        return NodeBatch(**fields)

    def _batch(self, seeds, input_id, step):
        from . import ops
        if self.prepare:
            if self.padded(seeds):
                self.load(seeds, step)
                return self.padded_batch(input_id)
            return self._prepared(seeds, input_id, step)
        d = self.data
        s = ops.sample_neighbors(self.csr, seeds, self.num_neighbors, seed=self.seed, step=step)
        A = s.adj
        n_idx = s.n_id.long()
        target = torch.repeat_interleave(torch.arange(A.n_rows, device=n_idx.device),
                                         (A.rowptr[1:] - A.rowptr[:-1]).long(), output_size=A.nnz)
        fields = dict(x=ops.pack_rows(d.x, s.n_id), edge_index=torch.stack([A.col[:A.nnz].long(), target]),
                      n_id=n_idx, adj=A, batch_size=s.batch_size, input_id=input_id,
                      num_sampled_nodes=s.num_sampled_nodes, num_sampled_edges=s.num_sampled_edges,
                      num_real_nodes=n_idx.numel())
        if getattr(d, "y", None) is not None:
            fields["y"] = d.y[n_idx]
        for name in _MASKS:
            mask = getattr(d, name, None)
            if mask is not None:
                fields[name] = mask[n_idx]
        return NodeBatch(**fields)
