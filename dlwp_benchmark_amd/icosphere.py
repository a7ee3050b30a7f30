"""Icospheres and the three GraphCast graphs (reference models/graphcast/utils/graph.py and graph_utils.py).

The generator subdivides an icosahedron: every face (a, b, c) becomes (a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)
with one new vertex per edge, appended after the old ones and pushed onto the unit sphere, so order k's vertices are a
prefix of order k + 1's (the multimesh indexes every order's faces into the finest vertex table, graph.py:100-112).  It
writes the reference's JSON schema: order_k_vertices / order_k_faces / order_k_face_centroid for k <= level and the empty
"vertices" / "faces" keys, which Graph.max_order counts (graph.py:79-81).  It is NOT pymesh's icosphere: orientation and
vertex order differ, so graphs built on it match the reference given the same mesh file, not given the same level.

    python -m dlwp_benchmark_amd.icosphere --level 3 --out icospheres_l3.json

`graphcast_graphs` builds the multimesh, grid->mesh and mesh->grid graphs and their node / edge features as the reference
does, vectorised: edges in the reference's order (the multimesh as dgl.to_bidirected's simple graph sorted by (src, dst)),
features in float32 with the reference's torch operations.  Grid node id = h * W + w.
"""
import argparse
import json

import numpy as np
import torch


def icospheres(level: int) -> dict:
    """{order_k_vertices, order_k_faces, order_k_face_centroid for k <= level, vertices: [], faces: []} as numpy arrays"""
    if level < 0:
        raise ValueError(f"icosphere level {level}: >= 0")
    phi = (1.0 + np.sqrt(5.0)) / 2.0
    v = np.array([[-1, phi, 0], [1, phi, 0], [-1, -phi, 0], [1, -phi, 0], [0, -1, phi], [0, 1, phi], [0, -1, -phi],
                  [0, 1, -phi], [phi, 0, -1], [phi, 0, 1], [-phi, 0, -1], [-phi, 0, 1]], dtype=np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10],
                  [8, 6, 7], [9, 8, 1]], dtype=np.int64)
    out = {}
    for k in range(level + 1):
        if k:
            v, f = _subdivide(v, f)
        out[f"order_{k}_vertices"] = v.copy()
        out[f"order_{k}_faces"] = f.copy()
        out[f"order_{k}_face_centroid"] = v[f].mean(axis=1)
    out["vertices"], out["faces"] = np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)
    return out


def _subdivide(v, f):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)
    key = np.sort(e, axis=1)
    uniq, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(3, -1)
    # new vertices in order of first appearance (face by face, edges ab, bc, ca), appended after the old ones
    order_seen = inv.T.reshape(-1)
    _, pos = np.unique(order_seen, return_index=True)
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[np.argsort(pos, kind="stable")] = np.arange(len(uniq))
    mid = v[uniq[np.argsort(rank)]].mean(axis=1)
    mid /= np.linalg.norm(mid, axis=1, keepdims=True)
    nv = np.concatenate([v, mid], axis=0)
    ab, bc, ca = (len(v) + rank[inv[i]] for i in range(3))
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    nf = np.stack([np.stack([a, ab, ca], 1), np.stack([b, bc, ab], 1), np.stack([c, ca, bc], 1), np.stack([ab, bc, ca], 1)],
                  axis=1).reshape(-1, 3)
    return nv, nf


def to_json(ico: dict) -> str:
    return json.dumps({k: np.asarray(v).tolist() for k, v in ico.items()})


def load(path: str) -> dict:
    with open(path, "r") as fh:
        d = json.load(fh)
    return {k: (np.array(v) if isinstance(v, list) else v) for k, v in d.items()}


def max_order(ico: dict) -> int:
    return len([k for k in ico if "faces" in k]) - 2


# ---- graph construction (graph_utils.py) ---------------------------------------------------------------------------------
def _deg2rad(x):
    return x * np.pi / 180


def _rad2deg(x):
    return x * 180 / np.pi


def latlon2xyz(latlon: torch.Tensor) -> torch.Tensor:
    ll = _deg2rad(latlon)
    lat, lon = ll[:, 0], ll[:, 1]
    return torch.stack((torch.cos(lat) * torch.cos(lon), torch.cos(lat) * torch.sin(lon), torch.sin(lat)), dim=1)


def xyz2latlon(xyz: torch.Tensor, unit: str = "deg") -> torch.Tensor:
    lat, lon = torch.arcsin(xyz[:, 2]), torch.arctan2(xyz[:, 1], xyz[:, 0])
    return torch.stack((_rad2deg(lat), _rad2deg(lon)), 1) if unit == "deg" else torch.stack((lat, lon), 1)


def _rotate(x, theta, axis):
    r = torch.zeros((theta.size(0), 3, 3))
    c, s = torch.cos(theta), torch.sin(theta)
    if axis == "y":
        r[:, 0, 0] += c
        r[:, 0, 2] += s
        r[:, 1, 1] += 1.0
        r[:, 2, 0] -= s
        r[:, 2, 2] += c
    else:
        r[:, 0, 0] += c
        r[:, 0, 1] -= s
        r[:, 1, 0] += s
        r[:, 1, 1] += c
        r[:, 2, 2] += 1.0
    return torch.matmul(r, x.unsqueeze(-1)).squeeze()


def edge_features(src_pos: torch.Tensor, dst_pos: torch.Tensor, src, dst) -> torch.Tensor:
    """add_edge_features (normalize=True): the source in the destination's local frame, / the largest displacement"""
    s, d = src_pos[torch.as_tensor(src).long()], dst_pos[torch.as_tensor(dst).long()]
    ll = xyz2latlon(d, unit="rad")
    lat, lon = ll[:, 0], ll[:, 1]
    az = torch.where(lon >= 0.0, 2 * np.pi - lon, -lon)
    po = torch.where(lat >= 0.0, lat, 2 * np.pi + lat)
    s, d = _rotate(s, az, "z"), _rotate(d, az, "z")
    s, d = _rotate(s, po, "y"), _rotate(d, po, "y")
    disp = s - d
    n = torch.linalg.norm(disp, dim=-1, keepdim=True)
    mx = torch.max(n)
    return torch.cat((disp / mx, n / mx), dim=-1)


def node_features(pos: torch.Tensor) -> torch.Tensor:
    """add_node_features: cos(lat), sin(lon), cos(lon) of the DEGREE values (the reference's xyz2latlon default unit)"""
    ll = xyz2latlon(pos)
    lat, lon = ll[:, 0], ll[:, 1]
    return torch.stack((torch.cos(lat), torch.sin(lon), torch.cos(lon)), dim=-1)


def lat_lon_grid(height: int, width: int) -> torch.Tensor:
    """graph_cast_net.py:190-194, flattened to [H * W, 2] (lat, lon), node h * W + w"""
    lat = torch.linspace(-90, 90, steps=height)
    lon = torch.linspace(-180, 180, steps=width + 1)[1:]
    g = torch.stack(torch.meshgrid(lat, lon, indexing="ij"), dim=-1)
    return g.permute(2, 0, 1).reshape(2, -1).permute(1, 0)


def _nearest(points, queries, k):
    try:
        from sklearn.neighbors import NearestNeighbors
    except ImportError as e:
        raise ImportError("GraphCastNet's grid<->mesh graphs use sklearn.neighbors.NearestNeighbors, as the reference does "
                          "(utils/graph.py:163, :219); scikit-learn is not installed") from e
    return NearestNeighbors(n_neighbors=k).fit(points).kneighbors(np.asarray(queries))


def graphcast_graphs(ico: dict, height: int, width: int) -> dict:
    """{"mesh" | "g2m" | "m2g": (src, dst, edge features [E, 4]), "mesh_nodes": [N_mesh, 3], "n_mesh": N_mesh}"""
    L = max_order(ico)
    verts = ico[f"order_{L}_vertices"]
    faces_l = ico[f"order_{L}_faces"]
    mesh_pos = torch.tensor(verts, dtype=torch.float32)
    # multimesh (create_mesh_graph): every order's faces, cell_to_adj, to_bidirected
    faces = np.concatenate([ico[f"order_{k}_faces"] for k in range(L + 1)]).astype(np.int64)
    pairs = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], axis=0)
    both = np.unique(np.concatenate([pairs, pairs[:, ::-1]], axis=0), axis=0)
    both = both[both[:, 0] != both[:, 1]]
    ms, md = both[:, 0], both[:, 1]
    out = {"mesh": (ms, md, edge_features(mesh_pos, mesh_pos, ms, md)), "mesh_nodes": node_features(mesh_pos),
           "n_mesh": len(verts)}
    grid = latlon2xyz(lat_lon_grid(height, width))
    # g2m (create_g2m_graph): 4 nearest order-L vertices within 0.6 x the longest face edge
    edge_len = max(np.max(np.linalg.norm(verts[faces_l[:, a]] - verts[faces_l[:, b]], axis=1))
                   for a, b in ((0, 1), (0, 2), (1, 2)))
    dist, idx = _nearest(verts, grid, 4)
    keep = (dist <= 0.6 * edge_len).reshape(-1)
    gs = np.repeat(np.arange(len(grid)), 4)[keep]
    gd = idx.reshape(-1)[keep]
    out["g2m"] = (gs, gd, edge_features(grid.to(torch.float32), mesh_pos, gs, gd))
    # m2g (create_m2g_graph): the three vertices of the face with the nearest centroid
    _, fi = _nearest(ico[f"order_{L}_face_centroid"], grid, 1)
    ts = faces_l[fi.reshape(-1)].reshape(-1)
    td = np.repeat(np.arange(len(grid)), 3)
    out["m2g"] = (ts, td, edge_features(mesh_pos, grid.to(torch.float32), ts, td))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="write an icosphere JSON in the GraphCast reference's schema")
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    with open(a.out, "w") as fh:
        fh.write(to_json(icospheres(a.level)))


if __name__ == "__main__":
    main()
