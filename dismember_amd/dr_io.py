"""Deep-Retrieval files.

The mapping file is the reference's (MappingOp.writeMapping / loadMapping, deep-retrieval/.../model/MappingOp.scala:45-94): a 4-byte
big-endian size, then one `ItemSet` message (deep-retrieval/src/main/protobuf/item_mapping.proto):

    ItemSet { repeated Item items = 1 }     Item { int32 item = 1; int32 id = 2; repeated Path paths = 3 }     Path { repeated int32 index = 1 }

read and written with the hand-written varint codec of tree_io (no protobuf runtime).  proto3 writes `index` packed and leaves out
zero scalars and empty packed fields; the reader also accepts the unpacked form.

The model file is this project's own: the reference saves its models with Java serialization, which stays out of scope.  Little-endian:

    magic "DMDRMODL" | int32 version (1) | int32 dtype (0 float32, 1 float64) | int32 E, L, K, D | int64 num_item | int32 rerank (0 / 1)
    layer_emb | layer_w[0] .. layer_w[D-1] | layer_b[0] .. layer_b[D-1] | rerank_emb | rerank_w | rerank_b | softmax_w | softmax_b

the arrays in dm_dr_model's order, the last five only when the flag is set.
"""
import struct

import numpy as np

from .tree_io import _f_bytes, _f_varint, _fields, _i32, _read_varint, _varint

MAGIC = b"DMDRMODL"
VERSION = 1
_HEADER = "<8siiiiiiqi"


# ------------------------------------------------------------------------------------------------------------------ the mapping file
def mapping_bytes(items, ids, paths):
    """items [n] original item ids, ids [n] internal ids, paths [n, J, D] (or a list of lists of lists) -> the file's bytes"""
    body = bytearray()
    for item, idx, ps in zip(np.asarray(items).tolist(), np.asarray(ids).tolist(), np.asarray(paths).tolist()):
        msg = _f_varint(1, item) + _f_varint(2, idx)
        for path in ps:
            packed = b"".join(_varint(v) for v in path)
            msg += _f_bytes(3, _f_bytes(1, packed), keep_empty=True)
        body += _f_bytes(1, msg, keep_empty=True)
    return struct.pack(">i", len(body)) + bytes(body)


def write_mapping(path, items, ids, paths):
    with open(path, "wb") as f:
        f.write(mapping_bytes(items, ids, paths))


def parse_mapping(data):
    """-> dict(items [n] int32, ids [n] int32, paths [n, J, D] int32), in file order"""
    (n,) = struct.unpack(">i", data[:4])
    if n < 0 or 4 + n > len(data):
        raise ValueError("mapping file: size prefix %d does not fit the file" % n)
    items, ids, paths = [], [], []
    for f, v in _fields(data[4:4 + n]):
        if f != 1:
            continue
        item = idx = 0
        ps = []
        for ff, vv in _fields(v):
            if ff == 1:
                item = _i32(vv)
            elif ff == 2:
                idx = _i32(vv)
            elif ff == 3:
                p = []
                for f3, v3 in _fields(vv):
                    if f3 != 1:
                        continue
                    if isinstance(v3, (bytes, bytearray)):          # packed
                        i = 0
                        while i < len(v3):
                            x, i = _read_varint(v3, i)
                            p.append(_i32(x))
                    else:
                        p.append(_i32(v3))
                ps.append(p)
        items.append(item); ids.append(idx); paths.append(ps)
    shapes = {(len(ps),) + tuple(len(p) for p in ps) for ps in paths}
    if len(shapes) > 1 or any(len(set(s[1:])) > 1 for s in shapes):
        raise ValueError("mapping file: items differ in their number of paths or the paths in their length")
    return dict(items=np.array(items, np.int32), ids=np.array(ids, np.int32), paths=np.array(paths, np.int32).reshape(len(items), -1, len(paths[0][0]) if paths and paths[0] else 0))


def read_mapping(path):
    with open(path, "rb") as f:
        return parse_mapping(f.read())


# ------------------------------------------------------------------------------------------------------------------ the model file
def save_model(path, engine):
    """the weights the engine holds (trained or loaded), read with dr_train_download("weights") and dr_rerank_download(.., "weights")"""
    from .dr_train import split_params, split_rerank
    from .engine import DismemberError
    d = engine.dr_dims
    E, L, K, D, ni, dt = d["E"], d["L"], d["K"], d["D"], d["num_item"], np.dtype(d["dtype"])
    w = split_params(engine.dr_train_download("weights"), E, L, K, D, ni)
    try:
        rr = split_rerank(engine.dr_rerank_download("graph"), engine.dr_rerank_download("softmax"), E, L, ni)
    except DismemberError as e:
        if e.code != -3:             # DM_ERR_STATE: the model was loaded without rerank arrays
            raise
        rr = None
    with open(path, "wb") as f:
        f.write(struct.pack(_HEADER, MAGIC, VERSION, 0 if dt == np.float32 else 1, E, L, K, D, ni, 1 if rr else 0))
        for a in [w["layer_emb"]] + list(w["layer_w"]) + list(w["layer_b"]):
            f.write(np.ascontiguousarray(a, dt.newbyteorder("<")).tobytes())
        if rr:
            for k in ("rerank_emb", "rerank_w", "rerank_b", "softmax_w", "softmax_b"):
                f.write(np.ascontiguousarray(rr[k], dt.newbyteorder("<")).tobytes())


def read_model(path):
    """-> (weights dict as Engine.dr_load_model takes it, dict(E, L, K, D, num_item, dtype))"""
    with open(path, "rb") as f:
        data = f.read()
    hs = struct.calcsize(_HEADER)
    magic, version, dtype, E, L, K, D, ni, rerank = struct.unpack(_HEADER, data[:hs])
    if magic != MAGIC or version != VERSION or dtype not in (0, 1):
        raise ValueError("%s is not a Deep-Retrieval model file of version %d" % (path, VERSION))
    dt = np.dtype("<f4" if dtype == 0 else "<f8")
    pos = [hs]

    def take(*shape):
        n = int(np.prod(shape))
        a = np.frombuffer(data, dt, n, pos[0]).reshape(shape)
        pos[0] += n * dt.itemsize
        return a
    w = dict(layer_emb=take(ni + K * (D - 1), E), layer_w=[take(K, (L + d) * E) for d in range(D)])
    w["layer_b"] = [take(K) for _ in range(D)]
    if rerank:
        w.update(rerank_emb=take(ni, E), rerank_w=take(E, L * E), rerank_b=take(E), softmax_w=take(ni, E), softmax_b=take(ni))
    if pos[0] != len(data):
        raise ValueError("%s: %d bytes where the header announces %d" % (path, len(data), pos[0]))
    return w, dict(E=E, L=L, K=K, D=D, num_item=ni, dtype=np.float32 if dtype == 0 else np.float64)


def load_model(engine, path):
    """reads the file into `engine` (dr_load_model) -> the dims dict"""
    w, d = read_model(path)
    engine.dr_load_model(w, d["E"], d["L"], d["K"], d["D"], d["num_item"], dtype=d["dtype"])
    return d
