"""MeshGraphNet -- drop-in for reference models/mgn/meshgraphnet.py:65-628 (registered as `MeshGraphNet`, config
configs/model/meshgraphnet.yaml).  Same constructor kwargs (:123-222), state-dict names, order and shapes (`device_buffer`
of the modulus `Module` base, `edge_encoder.model.*`, `node_encoder.model.*`, `node_decoder.model.*`,
`processor.processor_layers.{2i}.edge_mlp.model.*` / `{2i+1}.node_mlp.model.*`) and forward signature.

The graph is built on the host exactly as the reference builds it (`reference_graph`) and kept in non-persistent buffers in
CSC order by destination: one graph shared by the batch, sample b's nodes at offset b N.  No batched graph is built.

A rollout step is one node-encoder launch, processor_size x message_passing_steps fused processor-layer launches and one
decoder launch (csrc/mgn.hip).  The edge encoder's input is static, so its [E, D] output is computed once per weight version
and shared by the batch.  Like the reference (:412-423) every message-passing step restarts from the encoded edges; the
processor passes only its node features on.  The rollout is device resident and does NOT reproduce the reference's crash
on the second step (`.to()` on a list, :469-472) nor its per-step `.cpu()` (:487).

Training with gradients (`.train()` and autograd recording) runs the same kernels inside autograd Functions
(training.mgn_mlp / training.mgn_layer) whose backward is csrc/mgn_bwd.hip: each saves only its inputs and recomputes
the forward in LDS, and every gradient is bitwise reproducible.  In training each layer writes fresh x' / e' tensors (the
next layer's saved inputs) instead of the eval path's ping-pong and in-place buffers, and the edge encoder runs once per
`forward` through the differentiable MLP (not the eval-time cache), so its gradients from every step and message-passing
step accumulate.  This holds, by default, for processors up to TRAIN_FUSED_MAX_WIDTH (the measured crossover), and under
`set_fused_layers("always")` wherever the backward envelope (widths up to 64, ops.mgn_layer_backward_supported) holds
(`uses_hip_training`).  Elsewhere -- wider default processors, widths outside the envelope such as "always" at D > 64 --
training runs the torch composition of the same math (ops.mgn_mlp_torch / ops.mgn_layer_torch) under autograd, as eval
does for processors wider than FUSED_MAX_WIDTH.
DLWP_TRAIN_TORCH_BACKWARD=1 keeps the HIP forward and differentiates the torch composition instead (a cross-check).
"""
import functools

import numpy as np
import torch
from torch import nn

from .. import lib as _lib
from .. import ops
from .. import training
from ._base import StepBackbone

GRAPH_TYPES = ("grid_2d", "grid_2d_8stencil", "delaunay")
# Widest processor the step runs on the fused kernels by default.  Measured at B = 32 on 32x64:
# D = 34 / 48 / 64 are 2.7x / 1.25x / 1.47x faster than the torch composition, D = 96 / 128 / 470 are 0.82x / 0.74x / 0.10x
# (per 16-edge chunk the fused layer re-reads every weight of the edge MLP; the composition's GEMMs read them once).
# Wider layers take the composition unless `set_fused_layers("always")`; the kernels themselves run up to D = 512.
FUSED_MAX_WIDTH = 64
# Widest processor that TRAINS on the HIP kernels by default.  Measured at B = 32, sequence_length 3 (DESIGN.md section 16,
# profiles/meshgraphnet_train.jsonl): the yaml D = 34 step is 1.24x faster than the composition (1.12x on grid_2d 128x256),
# D = 48 / 64 with 15 layers are 0.75x / 0.52x.  Wider processors train on the composition unless
# `set_fused_layers("always")`; the backward kernels themselves run up to D = 64.
TRAIN_FUSED_MAX_WIDTH = 34


class MeshGraphMLP(nn.Module):
    """mesh_graph_mlp.py MeshGraphMLP: Linear, ReLU, (Linear, ReLU) x (hidden_layers - 1), Linear[, LayerNorm]"""

    def __init__(self, input_dim: int, output_dim: int, hidden_dim: int, hidden_layers: int, norm: bool = True):
        super().__init__()
        act = nn.ReLU()
        layers = [nn.Linear(input_dim, hidden_dim), act]
        for _ in range(hidden_layers - 1):
            layers += [nn.Linear(hidden_dim, hidden_dim), act]
        layers.append(nn.Linear(hidden_dim, output_dim))
        if norm:
            layers.append(nn.LayerNorm(output_dim))
        self.model = nn.Sequential(*layers)

    def forward(self, x):
        return self.model(x)


class MeshEdgeBlock(nn.Module):
    """mesh_edge_block.py with MeshGraphEdgeMLPConcat: e' = mlp([e, x_src, x_dst]) + e"""

    def __init__(self, dim: int, layers: int):
        super().__init__()
        self.edge_mlp = MeshGraphMLP(3 * dim, dim, dim, layers)


class MeshNodeBlock(nn.Module):
    """mesh_node_block.py: x' = mlp([aggregate(e'), x]) + x"""

    def __init__(self, aggregation: str, dim: int, layers: int):
        super().__init__()
        self.aggregation = aggregation
        self.node_mlp = MeshGraphMLP(2 * dim, dim, dim, layers)


class MeshGraphNetProcessor(nn.Module):
    """meshgraphnet.py:492-628: processor_size (edge block, node block) pairs in one ModuleList"""

    def __init__(self, processor_size: int, dim: int, num_layers_node: int, num_layers_edge: int, aggregation: str,
                 num_processor_checkpoint_segments: int = 0):
        super().__init__()
        self.processor_size = processor_size
        layers = []
        for _ in range(processor_size):
            layers += [MeshEdgeBlock(dim, num_layers_edge), MeshNodeBlock(aggregation, dim, num_layers_node)]
        self.processor_layers = nn.ModuleList(layers)
        self.num_processor_layers = len(layers)
        # a training-memory knob of the reference (:547-574); validated the same way, no effect on the arithmetic
        if num_processor_checkpoint_segments > 0 and self.num_processor_layers % num_processor_checkpoint_segments:
            raise ValueError("Processor layers must be a multiple of checkpoint_segments")
        self.num_processor_checkpoint_segments = num_processor_checkpoint_segments

    def pairs(self):
        layers = self.processor_layers
        return [(layers[2 * i].edge_mlp.model, layers[2 * i + 1].node_mlp.model) for i in range(self.processor_size)]


def _as_periodic(periodic):
    """bool, or a (rows, cols) pair from any non-string sequence (list, tuple, Hydra ListConfig) -- hashable"""
    if isinstance(periodic, (str, bytes)):
        raise ValueError(f"periodic {periodic!r}: a bool or a pair of bools")
    if hasattr(periodic, "__len__") and hasattr(periodic, "__getitem__"):
        if len(periodic) != 2:
            raise ValueError(f"periodic {list(periodic)!r}: a bool or a pair of bools")
        return bool(periodic[0]), bool(periodic[1])
    return bool(periodic)


def _periodic_pair(periodic):
    p = _as_periodic(periodic)
    return p if isinstance(p, tuple) else (p, p)


def _grid_edges(height: int, width: int, periodic) -> set:
    """undirected edges of networkx.grid_2d_graph(m=height, n=width, periodic) as (i, j) node-tuple pairs"""
    pr, pc = _periodic_pair(periodic)
    edges = set()
    for i in range(height):
        for j in range(width):
            if i + 1 < height:
                edges.add(((i, j), (i + 1, j)))
            if j + 1 < width:
                edges.add(((i, j), (i, j + 1)))
    if pr and height > 2:
        edges.update(((0, j), (height - 1, j)) for j in range(width))
    if pc and width > 2:
        edges.update(((i, 0), (i, width - 1)) for i in range(height))
    return edges


@functools.lru_cache(maxsize=None)
def _reference_graph(graph_type: str, height: int, width: int, periodic):
    h, w = height, width
    if graph_type in ("grid_2d", "grid_2d_8stencil"):
        und = _grid_edges(h, w, periodic)
        if graph_type == "grid_2d_8stencil":
            # :264-275: diagonal neighbours `(node + diagonals) % height` -- BOTH coordinates modulo the height (a quirk of
            # the reference, kept); a column index that leaves the grid would add nodes the forward cannot place
            if h > w:
                raise ValueError(f"grid_2d_8stencil with height {h} > width {w}: the reference's `% height` on the column "
                                 "adds nodes outside the grid")
            for i in range(h):
                for j in range(w):
                    for di, dj in ((-1, 1), (1, 1), (1, -1), (-1, -1)):
                        und.add(((i, j), ((i + di) % h, (j + dj) % h)))
        pairs = np.array([(a[0] * w + a[1], b[0] * w + b[1]) for a, b in und], dtype=np.int64).reshape(-1, 2)
        n_nodes = h * w
    elif graph_type == "delaunay":
        try:
            from scipy.spatial import Delaunay
        except ImportError as e:
            raise ImportError("MeshGraphNet(graph_type='delaunay') triangulates with scipy.spatial.Delaunay, as the reference "
                              "does (meshgraphnet.py:296); scipy is not installed") from e
        if not periodic:
            raise ValueError("delaunay with periodic=False has height * (width + 1) nodes: the reference's forward cannot "
                             "map them onto the height x width grid")
        xx, yy = np.meshgrid(np.arange(w + 1), np.arange(h))
        pts = np.stack((xx.flatten().astype(np.float32), yy.flatten().astype(np.float32)), axis=1)
        simp = Delaunay(pts).simplices.copy()
        for i in range(h):          # :301-303: the column x = width is the column x = 0
            simp[simp == (w + 1) * i + w] = (w + 1) * i
        pairs = np.concatenate([simp[:, [0, 1]], simp[:, [1, 2]], simp[:, [2, 0]]], axis=0).astype(np.int64)
        # labels y (w + 1) + x -> sorted relabel (dgl.from_networkx over a networkx graph) = y w + x
        pairs = (pairs // (w + 1)) * w + pairs % (w + 1)
        n_nodes = h * w
    else:
        raise ValueError(f"graph_type is '{graph_type}' but should be any of ['grid_2d', 'delaunay', 'grid_2d_8stencil'].")
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    both = np.concatenate([pairs, pairs[:, ::-1]], axis=0)                 # dgl.to_bidirected: simple symmetric graph
    both = np.unique(both, axis=0)
    src, dst = both[:, 0], both[:, 1]
    feats = _edge_features(src, dst, h, w, add_distance=graph_type == "grid_2d_8stencil")
    return n_nodes, src, dst, feats


def _edge_features(src, dst, height, width, add_distance):
    """create_edge_features (:317-345) with its quirks kept on purpose: the coordinates are (u // height, u % width), and
    the periodic fix-ups run one after the other, H-1 -> -1, W-1 -> -1, -(H-1) -> 1, -(W-1) -> 1, each on the result of
    the previous one"""
    u, v = src.astype(np.int64), dst.astype(np.int64)
    normal = np.stack([v // height - u // height, v % width - u % width], axis=1)
    normal[normal == height - 1] = -1
    normal[normal == width - 1] = -1
    normal[normal == -(height - 1)] = 1
    normal[normal == -(width - 1)] = 1
    feats = normal.astype(np.float32)
    if add_distance:
        dist = np.sqrt(np.abs(normal).sum(axis=1).astype(np.float32))
        feats = np.concatenate([feats, (dist / dist.max()).astype(np.float32)[:, None]], axis=1)
    return feats


def reference_graph(graph_type: str, height: int, width: int, periodic=True):
    """(n_nodes, src, dst, edge_features) of the reference's graph, edges sorted by (src, dst); node id = h * width + w"""
    return _reference_graph(graph_type, int(height), int(width), _as_periodic(periodic))


def _graph_attr(graph, name):
    if graph is None:
        raise ValueError("MeshGraphNet needs `graph` with height / width / periodic (configs/model/meshgraphnet.yaml)")
    return getattr(graph, name) if hasattr(graph, name) else graph[name]     # attribute object (DictConfig) or mapping


class MeshGraphNet(StepBackbone):
    def __init__(self, constant_channels: int = 4, prescribed_channels: int = 0, prognostic_channels: int = 1,
                 input_dim_edges: int = 2, context_size: int = 5, processor_size: int = 15, message_passing_steps: int = 1,
                 num_layers_node_processor: int = 2, num_layers_edge_processor: int = 2, hidden_dim_processor: int = 128,
                 hidden_dim_node_encoder: int = 128, num_layers_node_encoder: int = 2, hidden_dim_edge_encoder: int = 128,
                 num_layers_edge_encoder: int = 2, hidden_dim_node_decoder: int = 128, num_layers_node_decoder: int = 2,
                 aggregation: str = "sum", do_concat_trick: bool = False, num_processor_checkpoint_segments: int = 0,
                 graph_type: str = "grid_2d", **kwargs):
        super().__init__()
        if do_concat_trick:
            raise NotImplementedError("do_concat_trick=True (MeshGraphEdgeMLPSum) is not used by the reference config and "
                                      "has another parameter layout")
        if aggregation not in ("sum", "mean"):
            raise ValueError(f"aggregation {aggregation!r}: sum or mean")
        self.register_buffer("device_buffer", torch.empty(0))        # modulus Module (utils/module.py:78)
        self.context_size = int(context_size)
        self.message_passing_steps = int(message_passing_steps)
        self.aggregation = aggregation
        self.graph_type = graph_type
        self.prognostic_channels = prognostic_channels
        input_dim_nodes = constant_channels + (prescribed_channels + prognostic_channels) * context_size
        g = kwargs.get("graph")
        self.height, self.width = int(_graph_attr(g, "height")), int(_graph_attr(g, "width"))
        n_nodes, src, dst, feats = reference_graph(graph_type, self.height, self.width, _graph_attr(g, "periodic"))
        if feats.shape[1] != input_dim_edges:
            raise ValueError(f"input_dim_edges={input_dim_edges}, but the {graph_type} graph has {feats.shape[1]}-wide edge "
                             "features")
        self.n_nodes = n_nodes
        dim = hidden_dim_processor
        self.edge_encoder = MeshGraphMLP(input_dim_edges, dim, hidden_dim_edge_encoder, num_layers_edge_encoder)
        self.node_encoder = MeshGraphMLP(input_dim_nodes, dim, hidden_dim_node_encoder, num_layers_node_encoder)
        self.node_decoder = MeshGraphMLP(dim, prognostic_channels, hidden_dim_node_decoder, num_layers_node_decoder,
                                         norm=False)
        self.processor = MeshGraphNetProcessor(processor_size, dim, num_layers_node_processor, num_layers_edge_processor,
                                               aggregation, num_processor_checkpoint_segments)
        # the graph in CSC order by destination (non-persistent: not in the reference's state dict)
        order = np.lexsort((src, dst))
        src_c, dst_c = src[order], dst[order]
        deg = np.bincount(dst_c, minlength=n_nodes)
        row_ptr = np.concatenate([[0], np.cumsum(deg)])
        self.register_buffer("graph_row_ptr", torch.from_numpy(row_ptr.astype(np.int32)), persistent=False)
        self.register_buffer("graph_src", torch.from_numpy(src_c.astype(np.int32)), persistent=False)
        self.register_buffer("graph_dst", torch.from_numpy(dst_c.astype(np.int32)), persistent=False)
        self.register_buffer("graph_deg", torch.from_numpy(deg.astype(np.int32)), persistent=False)
        self.register_buffer("graph_edge_features", torch.from_numpy(np.ascontiguousarray(feats[order])), persistent=False)
        # the same edges sorted by source (a CSR by source over the CSC indices): the backward's source-side gather
        src_perm = np.argsort(src_c, kind="stable")
        src_row_ptr = np.concatenate([[0], np.cumsum(np.bincount(src_c, minlength=n_nodes))])
        self.register_buffer("graph_src_row_ptr", torch.from_numpy(src_row_ptr.astype(np.int32)), persistent=False)
        self.register_buffer("graph_src_perm", torch.from_numpy(src_perm.astype(np.int32)), persistent=False)
        self._pk = {}               # MeshGraphMLP -> ops.MgnMlpWeights (transposed weights)
        self._enc_edges = None      # (key, [E, D] encoded edge table)
        self.fused_layers = "auto"  # "auto": fused kernels up to FUSED_MAX_WIDTH; "always": everywhere they run
        self._bufs = None
        self._enc_train = None      # the edge encoder's output of the current training forward

    @property
    def n_edges(self) -> int:
        return int(self.graph_src.numel())

    def _packed(self, mlp: nn.Sequential) -> ops.MgnMlpWeights:
        p = self._pk.get(id(mlp))
        if p is None:
            p = self._pk[id(mlp)] = ops.MgnMlpWeights()
        return p

    def hip_supported(self) -> bool:
        """every MLP of the step inside the HIP kernels' envelope (ops.mgn_layer_supported / mgn_mlp_supported)"""
        return (ops.mgn_mlp_supported(self.node_encoder.model) and ops.mgn_mlp_supported(self.edge_encoder.model)
                and ops.mgn_mlp_supported(self.node_decoder.model)
                and all(ops.mgn_layer_supported(e, n, self.aggregation) for e, n in self.processor.pairs()))

    def set_fused_layers(self, mode: str):
        """"auto" (default): the fused kernels for processor widths up to FUSED_MAX_WIDTH (training: TRAIN_FUSED_MAX_WIDTH),
        the torch composition above; "always": the fused kernels wherever hip_supported() (training: wherever the backward
        envelope holds too)"""
        if mode not in ("auto", "always"):
            raise _lib.DlwpError(f"fused_layers {mode!r}: 'auto' or 'always'")
        self.fused_layers = mode
        self._graphed = None
        return self

    def uses_fused_layers(self) -> bool:
        dim = self.processor.processor_layers[0].edge_mlp.model[-1].normalized_shape[0]
        return self.hip_supported() and (self.fused_layers == "always" or dim <= FUSED_MAX_WIDTH)

    def backward_supported(self) -> bool:
        """every MLP of the step inside the backward kernels' envelope (ops.mgn_layer_backward_supported /
        mgn_mlp_backward_supported: widths up to 64)"""
        return (ops.mgn_mlp_backward_supported(self.node_encoder.model)
                and ops.mgn_mlp_backward_supported(self.edge_encoder.model)
                and ops.mgn_mlp_backward_supported(self.node_decoder.model)
                and all(ops.mgn_layer_backward_supported(e, n, self.aggregation) for e, n in self.processor.pairs()))

    def uses_hip_training(self) -> bool:
        """training with gradients runs the HIP forward and backward kernels (else the torch composition under autograd):
        processors up to TRAIN_FUSED_MAX_WIDTH by default, wherever the backward envelope holds under "always".
        """
        dim = self.processor.processor_layers[0].edge_mlp.model[-1].normalized_shape[0]
        return (self.uses_fused_layers() and self.backward_supported()
                and (self.fused_layers == "always" or dim <= TRAIN_FUSED_MAX_WIDTH))

    def _encoded_edges(self) -> torch.Tensor:
        key = self._param_key()
        if self._enc_edges is None or self._enc_edges[0] != key:
            ef = self.graph_edge_features
            self._enc_edges = (key, ops.mgn_mlp(self._packed(self.edge_encoder.model), self.edge_encoder.model, ef, 1,
                                                ef.shape[0]))
        return self._enc_edges[1]

    def _workspace_buffers(self, b: int, dim: int, device):
        key = (b, dim, str(device))
        if self._bufs is None or self._bufs[0] != key:
            n, e = self.n_nodes, self.n_edges
            self._bufs = (key, torch.empty(2, b * n, dim, device=device), torch.empty(b * e, dim, device=device))
        return self._bufs[1], self._bufs[2]

    def one_step(self, x_t: torch.Tensor) -> torch.Tensor:
        """x_t [B, C_in, H, W] -> increment [B, C_out, H, W] (update_nodes_and_edges, :412-423)"""
        b, _, h, w = x_t.shape
        if (h, w) != (self.height, self.width):
            raise _lib.DlwpError(f"input grid {h}x{w} does not match the graph's {self.height}x{self.width}")
        if self.training and torch.is_grad_enabled():
            return self._step_train(x_t) if self.uses_hip_training() else self._step_torch(x_t)
        if not self.uses_fused_layers():
            return self._step_torch(x_t)
        n = self.n_nodes
        dim = self.processor.processor_layers[0].edge_mlp.model[-1].normalized_shape[0]
        x = ops.mgn_mlp(self._packed(self.node_encoder.model), self.node_encoder.model, x_t, b, n, channels_first_in=True)
        enc = self._encoded_edges()
        xs, ebuf = self._workspace_buffers(b, dim, x_t.device)
        cur, k = x, 0
        for _ in range(self.message_passing_steps):
            for i, (em, nm) in enumerate(self.processor.pairs()):
                nxt = xs[k]
                k ^= 1
                ops.mgn_processor_layer(self._packed(em), em, self._packed(nm), nm, self.aggregation, self.graph_row_ptr,
                                        self.graph_src, self.graph_dst, b, cur, nxt, enc if i == 0 else ebuf, i == 0, ebuf)
                cur = nxt
        y = ops.mgn_mlp(self._packed(self.node_decoder.model), self.node_decoder.model, cur, b, n, channels_first_out=True)
        return y.view(b, self.prognostic_channels, h, w)

    def _graph_tuple(self):
        return (self.graph_row_ptr, self.graph_src, self.graph_dst, self.graph_deg, self.graph_src_row_ptr,
                self.graph_src_perm)

    def _encode_edges_train(self) -> torch.Tensor:
        """the edge encoder through the differentiable MLP (not the eval cache: its parameters take gradients)"""
        ef = self.graph_edge_features
        return training.mgn_mlp(self.edge_encoder.model, self._packed(self.edge_encoder.model), ef, 1, ef.shape[0])

    def _step_train(self, x_t: torch.Tensor) -> torch.Tensor:
        """one step with autograd on the HIP kernels: every MLP and processor layer is an autograd Function whose backward
        runs csrc/mgn_bwd.hip; each layer writes fresh x' / e' (the next layer's saved inputs)"""
        b, _, h, w = x_t.shape
        n = self.n_nodes
        enc = self._enc_train if self._enc_train is not None else self._encode_edges_train()
        x = training.mgn_mlp(self.node_encoder.model, self._packed(self.node_encoder.model), x_t, b, n,
                             channels_first_in=True)
        graph = self._graph_tuple()
        for _ in range(self.message_passing_steps):
            e, shared = enc, True
            for em, nm in self.processor.pairs():
                x, e = training.mgn_layer(em, self._packed(em), nm, self._packed(nm), self.aggregation, graph, b, x, e,
                                          shared)
                shared = False
        y = training.mgn_mlp(self.node_decoder.model, self._packed(self.node_decoder.model), x, b, n,
                             channels_first_out=True)
        return y.view(b, self.prognostic_channels, h, w)

    def _forward_train(self, constants, prescribed, prognostic):
        """the edge encoder runs once per forward; its gradients from every step and message-passing step accumulate"""
        if not self.uses_hip_training():
            return super()._forward_train(constants, prescribed, prognostic)
        self._enc_train = self._encode_edges_train()
        try:
            return super()._forward_train(constants, prescribed, prognostic)
        finally:
            self._enc_train = None

    def _step_torch(self, x_t: torch.Tensor) -> torch.Tensor:
        """the same step as a torch composition (autograd; widths outside the HIP envelope)"""
        b, c, h, w = x_t.shape
        x = ops.mgn_mlp_torch(self.node_encoder.model, x_t.permute(0, 2, 3, 1).reshape(b * h * w, c))
        enc = ops.mgn_mlp_torch(self.edge_encoder.model, self.graph_edge_features)
        for _ in range(self.message_passing_steps):
            e = enc
            for em, nm in self.processor.pairs():
                x, e = ops.mgn_layer_torch(em, nm, self.aggregation, self.graph_src, self.graph_dst, self.graph_deg, b, x, e)
        y = ops.mgn_mlp_torch(self.node_decoder.model, x)
        return y.view(b, h, w, -1).permute(0, 3, 1, 2)
