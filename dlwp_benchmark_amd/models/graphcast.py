"""GraphCastNet -- drop-in for reference models/graphcast/graph_cast_net.py (commented out of the reference registry,
config configs/model/graphcast.yaml).  Same constructor kwargs, state-dict names, order and shapes (`device_buffer` of the
modulus `Module` base, `encoder_embedder.*`, `decoder_embedder.*`, `encoder.*`, `processor_encoder.*`, `processor.*`,
`processor_decoder.*`, `decoder.*`, `finale.*`) and forward signature.

The mesh is read from `meshgraph_path` when it exists; otherwise it is generated in memory (dlwp_benchmark_amd.icosphere)
at the level of an `_l<k>` suffix of the path, else 6.  The three graphs are built on the host as the reference builds
them and kept in non-persistent buffers in CSC order by destination, one graph shared by the batch.

A step runs every MLP on the gather-GEMM of csrc/graphcast.hip (ops.gc_mlp): the first Linear of an edge MLP is split into
W_e e + (W_s x_src)[src] + (W_d x_dst)[dst] with the node products computed once per node, and the node MLPs read
[aggregate, x] in the A-operand load.  The four static embeddings (mesh nodes, mesh / g2m / m2g edges) depend on the
weights only and are computed once per weight version.  Batches B >= 1 share the graph (the reference raises for B != 1).

Training with gradients (`.train()` and autograd recording) can run the same kernels inside autograd Functions
(training.gc_mlp / training.gc_layer) whose backward is csrc/graphcast_bwd.hip: each saves its inputs, every hidden
pre-activation and the LayerNorm input (the LayerNorm writes a fresh tensor), about half of what autograd of the
composition keeps, and every gradient is bitwise reproducible.  The static embeddings then run once per `forward`
through the Functions, so their gradients accumulate over the rollout steps.  The HIP backward is slower than the
composition at the benchmarked shapes, so training keeps the composition by default and
`set_hip_training(True)` opts in for the memory (`uses_hip_training`).  The composition (`_step_torch`) also trains MLPs
outside the envelope (ops.gc_mlp_supported, or no LayerNorm), `set_hip_step(False)` models and CPU tensors; eval MLPs
outside the envelope and `set_hip_step(False)` (A/B timing) run it too.  DLWP_TRAIN_TORCH_BACKWARD=1 keeps the HIP
forward and differentiates the composition instead (a cross-check).  The three forms share one walk of the step
(`_step`), given the MLP and layer functions of ops, training or the composition.
"""
import os
import re
from typing import Optional

import numpy as np
import torch
from torch import nn

from .. import icosphere
from .. import lib as _lib
from .. import ops
from .. import training
from ._base import StepBackbone

_ACTIVATIONS = {"relu": nn.ReLU, "leaky_relu": (nn.LeakyReLU, {"negative_slope": 0.1}), "relu6": nn.ReLU6, "elu": nn.ELU,
                "selu": nn.SELU, "silu": nn.SiLU, "gelu": nn.GELU, "sigmoid": nn.Sigmoid, "logsigmoid": nn.LogSigmoid,
                "softplus": nn.Softplus, "softshrink": nn.Softshrink, "softsign": nn.Softsign, "tanh": nn.Tanh,
                "tanhshrink": nn.Tanhshrink, "threshold": (nn.Threshold, {"threshold": 1.0, "value": 1.0}),
                "hardtanh": nn.Hardtanh}


def get_activation(name: str) -> nn.Module:
    """utils/activations.py get_activation for its parameter-free torch entries"""
    m = _ACTIVATIONS.get(name.lower())
    if m is None:
        raise NotImplementedError(f"activation {name!r}: one of {sorted(_ACTIVATIONS)}")
    return m[0](**m[1]) if isinstance(m, tuple) else m()


class MeshGraphMLP(nn.Module):
    """mesh_graph_mlp.py MeshGraphMLP: Linear, act, (Linear, act) x (hidden_layers - 1), Linear[, LayerNorm]"""

    def __init__(self, input_dim, output_dim, hidden_dim, hidden_layers, activation_fn, norm_type="LayerNorm"):
        super().__init__()
        layers = [nn.Linear(input_dim, hidden_dim), activation_fn]
        for _ in range(hidden_layers - 1):
            layers += [nn.Linear(hidden_dim, hidden_dim), activation_fn]
        layers.append(nn.Linear(hidden_dim, output_dim))
        if norm_type is not None:
            if norm_type != "LayerNorm":
                raise NotImplementedError(f"norm_type {norm_type!r}: LayerNorm or None (the only ones nn can build)")
            layers.append(nn.LayerNorm(output_dim))
        self.model = nn.Sequential(*layers)

    def forward(self, x):
        return self.model(x)


class _Embedder(nn.Module):
    def __init__(self, names_dims, d, hl, act, norm):
        super().__init__()
        for name, din in names_dims:
            setattr(self, name, MeshGraphMLP(din, d, d, hl, act, norm))


class _EdgeBlock(nn.Module):
    """mesh_edge_block.py with MeshGraphEdgeMLPConcat"""

    def __init__(self, d, hl, act, norm):
        super().__init__()
        self.edge_mlp = MeshGraphMLP(3 * d, d, d, hl, act, norm)


class _NodeBlock(nn.Module):
    def __init__(self, d, hl, act, norm):
        super().__init__()
        self.node_mlp = MeshGraphMLP(2 * d, d, d, hl, act, norm)


class GraphCastProcessor(nn.Module):
    def __init__(self, n, d, hl, act, norm):
        super().__init__()
        layers = []
        for _ in range(n):
            layers += [_EdgeBlock(d, hl, act, norm), _NodeBlock(d, hl, act, norm)]
        self.processor_layers = nn.ModuleList(layers)

    def pairs(self):
        ls = self.processor_layers
        return [(ls[2 * i].edge_mlp.model, ls[2 * i + 1].node_mlp.model) for i in range(len(ls) // 2)]


class MeshGraphEncoder(nn.Module):
    def __init__(self, d, hl, act, norm):
        super().__init__()
        self.edge_mlp = MeshGraphMLP(3 * d, d, d, hl, act, norm)
        self.src_node_mlp = MeshGraphMLP(d, d, d, hl, act, norm)
        self.dst_node_mlp = MeshGraphMLP(2 * d, d, d, hl, act, norm)


class MeshGraphDecoder(nn.Module):
    def __init__(self, d, hl, act, norm):
        super().__init__()
        self.edge_mlp = MeshGraphMLP(3 * d, d, d, hl, act, norm)
        self.node_mlp = MeshGraphMLP(2 * d, d, d, hl, act, norm)


# Training with gradients runs the HIP kernels only when opted in (set_hip_training): at the benchmarked shapes the HIP
# step is slower than the composition; it keeps about half the activation memory (DESIGN.md section 17,
# profiles/graphcast_train.jsonl).
HIP_TRAINING_DEFAULT = False


def _mesh_level(path: str) -> int:
    m = re.search(r"_l(\d+)", os.path.basename(str(path)))
    return int(m.group(1)) if m else 6


def _csc(src, dst, n_dst):
    """edge permutation into CSC order by destination (source order within), row_ptr [n_dst + 1]"""
    order = np.lexsort((src, dst))
    deg = np.bincount(dst[order], minlength=n_dst)
    return order, np.concatenate([[0], np.cumsum(deg)]).astype(np.int32), deg


class GraphCastNet(StepBackbone):
    def __init__(self, meshgraph_path: str, input_height: int = 721, input_width: int = 1440, constant_channels: int = 4,
                 prescribed_channels: int = 1, prognostic_channels: int = 8, input_dim_mesh_nodes: int = 3,
                 input_dim_edges: int = 4, processor_layers: int = 16, hidden_layers: int = 1, hidden_dim: int = 512,
                 aggregation: str = "sum", activation_fn: str = "silu", norm_type: str = "LayerNorm",
                 use_cugraphops_encoder: bool = False, use_cugraphops_processor: bool = False,
                 use_cugraphops_decoder: bool = False, do_concat_trick: bool = False, recompute_activation: bool = False,
                 partition_size: int = 1, partition_group_name: Optional[str] = None, expect_partitioned_input: bool = False,
                 produce_aggregated_output: bool = True, context_size: int = 1, **kwargs):
        super().__init__()
        if do_concat_trick:
            raise NotImplementedError("do_concat_trick=True (MeshGraphEdgeMLPSum) has another parameter layout")
        if use_cugraphops_encoder or use_cugraphops_processor or use_cugraphops_decoder:
            raise NotImplementedError("use_cugraphops_*: cugraph-ops is a CUDA library; the graphs here are HIP CSC tables")
        if partition_size > 1:
            raise NotImplementedError("partition_size > 1: distributed graph partitioning is not implemented")
        if processor_layers <= 2:
            raise ValueError("Expected at least 3 processor layers")
        if aggregation not in ("sum", "mean"):
            raise ValueError(f"aggregation {aggregation!r}: sum or mean")
        self.register_buffer("device_buffer", torch.empty(0))        # modulus Module (utils/module.py)
        self.context_size = int(context_size)
        self.aggregation = aggregation
        self.height, self.width = int(input_height), int(input_width)
        self.prognostic_channels = int(prognostic_channels)
        self.constant_channels, self.prescribed_channels = int(constant_channels), int(prescribed_channels)
        self.input_dim_grid_nodes = constant_channels + (prescribed_channels + prognostic_channels) * context_size
        d, hl = int(hidden_dim), int(hidden_layers)
        act = get_activation(activation_fn)                          # one instance shared by every MLP, as the reference

        if meshgraph_path is not None and os.path.exists(str(meshgraph_path)):
            ico = icosphere.load(str(meshgraph_path))
        else:
            ico = icosphere.icospheres(_mesh_level(meshgraph_path))
        g = icosphere.graphcast_graphs(ico, self.height, self.width)

        self.encoder_embedder = _Embedder([("grid_node_mlp", self.input_dim_grid_nodes), ("mesh_node_mlp", input_dim_mesh_nodes),
                                           ("mesh_edge_mlp", input_dim_edges), ("grid2mesh_edge_mlp", input_dim_edges)],
                                          d, hl, act, norm_type)
        self.decoder_embedder = _Embedder([("mesh2grid_edge_mlp", input_dim_edges)], d, hl, act, norm_type)
        self.encoder = MeshGraphEncoder(d, hl, act, norm_type)
        self.processor_encoder = GraphCastProcessor(1, d, hl, act, norm_type)
        self.processor = GraphCastProcessor(processor_layers - 2, d, hl, act, norm_type)
        self.processor_decoder = GraphCastProcessor(1, d, hl, act, norm_type)
        self.decoder = MeshGraphDecoder(d, hl, act, norm_type)
        self.finale = MeshGraphMLP(d, self.prognostic_channels, d, hl, act, None)

        self.n_mesh, self.n_grid = int(g["n_mesh"]), self.height * self.width
        self.register_buffer("mesh_ndata", g["mesh_nodes"].float().contiguous(), persistent=False)
        for name, n_dst in (("mesh", self.n_mesh), ("g2m", self.n_mesh), ("m2g", self.n_grid)):
            src, dst, feat = g[name]
            order, row_ptr, deg = _csc(np.asarray(src), np.asarray(dst), n_dst)
            self.register_buffer(f"{name}_src", torch.from_numpy(np.asarray(src)[order].astype(np.int32)), persistent=False)
            self.register_buffer(f"{name}_dst", torch.from_numpy(np.asarray(dst)[order].astype(np.int32)), persistent=False)
            self.register_buffer(f"{name}_row_ptr", torch.from_numpy(row_ptr), persistent=False)
            self.register_buffer(f"{name}_deg", torch.from_numpy(deg.astype(np.int32)), persistent=False)
            self.register_buffer(f"{name}_edata", feat[torch.from_numpy(order)].float().contiguous(), persistent=False)
        # channel order of the rollout's x_t ([constants, prescribed window, prognostic window]) -> the reference's
        # prepare_inputs order ([prescribed window, prognostic window, constants], graph_cast_net.py:691-694)
        cc, pw = self.constant_channels, (self.prescribed_channels + self.prognostic_channels) * self.context_size
        ref_order = torch.cat([torch.arange(cc, cc + pw), torch.arange(cc)])
        self.register_buffer("_to_ref_order", ref_order, persistent=False)
        self.register_buffer("_from_ref_order", torch.argsort(ref_order), persistent=False)   # rows of the grid embedder
        self._pk = {}
        self._static = None
        self._static_train = None   # the static embeddings of the current training forward
        self._graphs = {}
        self.hip_step = True
        self.hip_training = HIP_TRAINING_DEFAULT

    # ---- bookkeeping ---------------------------------------------------------------------------------------------------
    def _layer_mlps(self):
        """the (edge, node) MLP `model`s of every message-passing layer in step order: grid -> mesh, the processor layers,
        mesh -> grid"""
        enc, dec = self.encoder, self.decoder
        return ([(enc.edge_mlp.model, enc.dst_node_mlp.model)]
                + [pair for p in (self.processor_encoder, self.processor, self.processor_decoder) for pair in p.pairs()]
                + [(dec.edge_mlp.model, dec.node_mlp.model)])

    def _mlps(self):
        ee, de = self.encoder_embedder, self.decoder_embedder
        yield from (ee.grid_node_mlp.model, ee.mesh_node_mlp.model, ee.mesh_edge_mlp.model, ee.grid2mesh_edge_mlp.model,
                    de.mesh2grid_edge_mlp.model, self.encoder.src_node_mlp.model, self.finale.model)
        for pair in self._layer_mlps():
            yield from pair

    def hip_supported(self) -> bool:
        return all(ops.gc_mlp_supported(m) for m in self._mlps())

    def set_hip_step(self, on: bool = True):
        """True (default): the step on csrc/graphcast.hip wherever hip_supported(); False: the torch composition"""
        self.hip_step = bool(on)
        self._graphed = None
        return self

    def uses_hip_step(self) -> bool:
        return self.hip_step and self.hip_supported()

    def set_hip_training(self, on: bool = True):
        """True: training with gradients runs the HIP forward and backward kernels wherever uses_hip_training() holds;
        False (default, the faster path at the measured shapes): the torch composition under autograd"""
        self.hip_training = bool(on)
        return self

    def uses_hip_training(self) -> bool:
        """training with gradients runs on csrc/graphcast.hip + csrc/graphcast_bwd.hip: opted in, the HIP step on, every
        MLP inside the envelope (ops.gc_mlp_supported) and every message-passing MLP ending in its LayerNorm"""
        return (self.hip_training and self.uses_hip_step()
                and all(ops.mgn_parts(m)[1] is not None for pair in self._layer_mlps() for m in pair))

    def _packed(self, seq, split=None, perm=None) -> ops.GcMlpWeights:
        p = self._pk.get(id(seq))
        if p is None:
            p = self._pk[id(seq)] = ops.GcMlpWeights(split, perm)
        return p.get(seq)

    def _edge_packed(self, seq):
        d = seq[0].in_features // 3
        return self._packed(seq, split=(d, d, d))

    def _graph(self, name: str) -> dict:
        """graph `name` ("mesh", "g2m", "m2g") as the layers take it (training.gc_layer): row_ptr, src, dst, deg (CSC by
        destination), src_row_ptr, src_perm (ops.mgn_source_csr), n_src, n_dst; rebuilt when the buffers are replaced
        (.to(device))"""
        src = getattr(self, f"{name}_src")
        g = self._graphs.get(name)
        if g is None or g["src"] is not src:
            n_src, n_dst = {"mesh": (self.n_mesh, self.n_mesh), "g2m": (self.n_grid, self.n_mesh),
                            "m2g": (self.n_mesh, self.n_grid)}[name]
            src_row_ptr, src_perm = ops.mgn_source_csr(src, n_src)
            g = self._graphs[name] = dict(row_ptr=getattr(self, f"{name}_row_ptr"), src=src, dst=getattr(self, f"{name}_dst"),
                                          deg=getattr(self, f"{name}_deg"), src_row_ptr=src_row_ptr, src_perm=src_perm,
                                          n_src=n_src, n_dst=n_dst)
        return g

    # ---- the step --------------------------------------------------------------------------------------------------------
    def _step(self, x_t: torch.Tensor, mlp, layer, table) -> torch.Tensor:
        """the step, on one of three sets of functions:
        mlp(seq, x, batch, rows, mode=0, x_bs=None, residual=False, out_cf=False): one MLP in the layouts of
            training.gc_mlp (mode 1: the grid embedder on the channels-first input, in the rollout's channel order);
        layer(edge_seq, node_seq, graph name, batch, e, xs, xd, residual) -> (x', e'): one message-passing layer;
        table(name): the static embedding `name` (_static_table), asked for where the step first reads it"""
        b = x_t.shape[0]
        G = self.n_grid
        grid = mlp(self.encoder_embedder.grid_node_mlp.model, x_t.contiguous(), b, G, mode=1)
        g2m, *processor, m2g = self._layer_mlps()
        # grid -> mesh (mesh_graph_encoder.py): edge MLP without residual, dst node MLP + mesh_n, src node MLP + grid;
        # an edge output no later layer reads is not bound, so it is freed as soon as its layer returns
        mesh = layer(*g2m, "g2m", b, table("g2m_e"), grid, table("mesh_n"), False)[0]
        grid = mlp(self.encoder.src_node_mlp.model, grid, b, G, residual=True)
        # processor: processor_encoder, processor, processor_decoder (its edge output is discarded)
        e = table("mesh_e")
        for em, nm in processor:
            mesh, e = layer(em, nm, "mesh", b, e, mesh, mesh, True)
        # mesh -> grid (mesh_graph_decoder.py), then the norm-free finale, channels-first
        grid = layer(*m2g, "m2g", b, table("m2g_e"), mesh, grid, False)[0]
        y = mlp(self.finale.model, grid, b, G, out_cf=True)
        return y.view(b, self.prognostic_channels, self.height, self.width)

    def _static_table(self, mlp, name: str) -> torch.Tensor:
        """one static embedding (mesh nodes, mesh / g2m / m2g edges): a [rows, D] table the batch shares"""
        ee = self.encoder_embedder
        m, x = {"mesh_n": (ee.mesh_node_mlp, self.mesh_ndata), "mesh_e": (ee.mesh_edge_mlp, self.mesh_edata),
                "g2m_e": (ee.grid2mesh_edge_mlp, self.g2m_edata),
                "m2g_e": (self.decoder_embedder.mesh2grid_edge_mlp, self.m2g_edata)}[name]
        return mlp(m.model, x, 1, x.shape[0], x_bs=0)

    def _static_tables(self, mlp) -> dict:
        return {k: self._static_table(mlp, k) for k in ("mesh_n", "mesh_e", "g2m_e", "m2g_e")}

    # HIP step: ops.gc_mlp / ops.gc_layer, the static embeddings once per weight version
    def _hip_mlp(self, seq, x, batch, rows, mode=0, x_bs=None, residual=False, out_cf=False):
        x_bs = x.numel() // batch if x_bs is None else x_bs
        pk = self._packed(seq, perm=self._from_ref_order if mode == 1 else None)
        return ops.gc_mlp(pk, seq, batch, rows, ops.gc_a_fields(mode, x, x_bs), res=x if residual else None,
                          res_bs=x_bs if residual else 0, out_cf=out_cf)

    def _step_hip(self, x_t: torch.Tensor) -> torch.Tensor:
        key = self._param_key()
        if self._static is None or self._static[0] != key:
            self._static = (key, self._static_tables(self._hip_mlp))
        st = self._static[1]

        def layer(edge, node, name, b, e, xs, xd, residual):
            g = self._graph(name)
            # batch strides: 0 for the static tables, which the batch shares (at B = 1 too)
            bs = [0 if any(t is s for s in st.values()) else rows * t.shape[-1]
                  for t, rows in ((e, g["src"].numel()), (xs, g["n_src"]), (xd, g["n_dst"]))]
            return ops.gc_layer(self._edge_packed(edge), edge, self._packed(node), node, self.aggregation, g, b, e, xs, xd,
                                bs, residual)

        return self._step(x_t, self._hip_mlp, layer, st.__getitem__)

    # HIP training step: training.gc_mlp / training.gc_layer, the static embeddings once per forward
    def _train_mlp(self, seq, x, batch, rows, mode=0, x_bs=None, residual=False, out_cf=False):
        perm, col_order = (self._from_ref_order, self._to_ref_order) if mode == 1 else (None, None)
        return training.gc_mlp(seq, self._packed(seq, perm=perm), x, batch, rows, mode, x_bs, residual, out_cf, col_order)

    def _train_layer(self, edge, node, name, b, e, xs, xd, residual):
        return training.gc_layer(edge, self._edge_packed(edge), node, self._packed(node), self.aggregation,
                                 self._graph(name), b, e, xs, xd, residual)

    def _step_train(self, x_t: torch.Tensor) -> torch.Tensor:
        st = self._static_train if self._static_train is not None else self._static_tables(self._train_mlp)
        return self._step(x_t, self._train_mlp, self._train_layer, st.__getitem__)

    def _forward_train(self, constants, prescribed, prognostic):
        """the static embeddings once per forward (their gradients accumulate over the rollout steps), then the rollout"""
        if not (prognostic.is_cuda and self.uses_hip_training()):
            return super()._forward_train(constants, prescribed, prognostic)
        self._static_train = self._static_tables(self._train_mlp)
        try:
            return super()._forward_train(constants, prescribed, prognostic)
        finally:
            self._static_train = None

    # torch composition (autograd; outside the envelope): training.gc_mlp_torch / training.gc_layer_torch, concat-
    # materialising like the reference, each static embedding every step where it is read (so autograd runs its
    # backward as soon as its gradient is complete)
    def _torch_mlp(self, seq, x, batch, rows, mode=0, x_bs=None, residual=False, out_cf=False):
        return training.gc_mlp_torch(seq, x, batch, rows, mode, x_bs, residual, out_cf, self._to_ref_order)

    def _torch_layer(self, edge, node, name, b, e, xs, xd, residual):
        return training.gc_layer_torch(edge, node, self.aggregation, self._graph(name), b, e, xs, xd, residual)

    def _step_torch(self, x_t: torch.Tensor) -> torch.Tensor:
        return self._step(x_t, self._torch_mlp, self._torch_layer, lambda name: self._static_table(self._torch_mlp, name))

    # ---- rollout ---------------------------------------------------------------------------------------------------------
    def one_step(self, x_t: torch.Tensor) -> torch.Tensor:
        """x_t [B, C_in, H, W] (rollout channel order) -> increment [B, C_out, H, W] (forward_one_step)"""
        b, c, h, w = x_t.shape
        if (h, w) != (self.height, self.width) or c != self.input_dim_grid_nodes:
            raise _lib.DlwpError(f"input {c}x{h}x{w} does not match the model's {self.input_dim_grid_nodes}x{self.height}x"
                                 f"{self.width}")
        if self.training and torch.is_grad_enabled():
            if x_t.is_cuda and self.uses_hip_training():
                return self._step_train(x_t)
            return self._step_torch(x_t)
        if not self.uses_hip_step():
            return self._step_torch(x_t)
        return self._step_hip(x_t)

    def _check_inputs(self, constants, prescribed, prognostic):
        constants, prescribed, prognostic = super()._check_inputs(constants, prescribed, prognostic)
        return (None if self.constant_channels == 0 else constants), prescribed, prognostic
