"""EmbeddingVariable checkpoints in DeepRec's on-disk layout.

Two layers:

* `BundleWriter` / `BundleReader`: TensorFlow's TensorBundle V2 format
  (core/util/tensor_bundle/tensor_bundle.cc) -- `<prefix>.data-00000-of-00001`
  holds the tensors' raw little-endian bytes in the order they were added,
  `<prefix>.index` is an SSTable (core/lib/io/table_builder.cc, LevelDB
  format: 256 KiB blocks, restart interval 16, no compression, masked crc32c
  block trailers) mapping "" -> BundleHeaderProto and each tensor name ->
  BundleEntryProto {dtype, shape, shard_id, offset, size, masked crc32c}
  (core/protobuf/tensor_bundle.proto).  The writer reproduces the reference's
  files byte for byte (tests/golden/ckpt/, from the reference's testdata).

* `dump_embedding_values` / `restore_embedding_variable`: what DeepRec's
  saver ops do for an EV (core/kernels/kv_variable_ops.h:148-265 and
  :459-673, save_restore_v2_ops.cc:128-133).  Save writes
  `<name>-partition_offset` (int32 [1001]) and `<name>-{keys, values,
  versions, freqs}` with the keys grouped into kSavedPartitionNum = 1000
  sub-partitions by `key % 1000` (C++ remainder: negative keys match no
  sub-partition and are not saved), so a job with a different partition
  count can restore its share.  Restore follows EVRestoreDynamically: a name
  without "part_" imports everything; otherwise the new form (partition
  offsets present) reads, from every saved part, the sub-partitions
  i % partition_num == partition_id, and the old form reads whole parts;
  both import through EmbeddingVar::Import with the
  `key % 1000 % partition_num == partition_id` filter, versions default -1
  and freqs default to filter_freq (MinFreq).

The device side is the engine's: `EmbeddingVariable.export()` (dr_ev_export,
GPU), the 1000-way stable split (dr_partition_by_owner with world = 1000 +
dr_rows_pack, GPU) and `import_partitioned()` (dr_ev_insert, GPU).  Only the
file bytes pass through the host; checksums run natively (dr_crc32c_extend).
Values keep the EV's dtype on disk: DT_FLOAT, DT_DOUBLE, or DT_BFLOAT16 for a
bf16 EV (build-defined, like the bf16 EV itself).

Beside EVs the four entry points take DenseTables (one whole entry per table,
as a tf.Variable is written; NAME-sparse_incr_{keys, values} in a delta),
MultiHashVariables and AdaptiveEmbeddingVariables (their members,
expand_variables) and the objects of optimizer.checkpoint_variables: slot
EVs, dense slots and the beta-power scalars.
"""
import os
import struct

import numpy as np
import torch

from . import _lib

SAVED_PARTITION_NUM = 1000            # kv_variable_ops.h:39
_MAGIC = 0xdb4775248b80fb57           # table/format.h kTableMagicNumber
_BLOCK_SIZE = 262144                  # core/lib/io/table_options.h:41
_RESTART_INTERVAL = 16                # :46

_DT = {np.dtype(np.float32): 1, np.dtype(np.float64): 2, np.dtype(np.int32): 3,
       np.dtype(np.uint8): 4, np.dtype(np.int16): 5, np.dtype(np.int8): 6,
       np.dtype(np.int64): 9, np.dtype(np.bool_): 10, np.dtype(np.uint16): 17,
       np.dtype(np.float16): 19, np.dtype(np.uint32): 22, np.dtype(np.uint64): 23}
_NP = {v: k for k, v in _DT.items()}
# DT_BFLOAT16 (types.proto): numpy has no bfloat16, so the rows of a bf16 EV
# pass through the host as their raw 16-bit patterns -- written from a torch
# bfloat16 tensor, read back as uint16 and viewed as bfloat16 by the import
_DT_BFLOAT16 = 14
_NP[_DT_BFLOAT16] = np.dtype(np.uint16)


def crc32c(data, init=0):
    """crc32c::Extend (core/lib/hash/crc32c.h), native."""
    if isinstance(data, np.ndarray):
        data = np.ascontiguousarray(data)
        return _lib.lib().dr_crc32c_extend(init, data.ctypes.data, data.nbytes)
    return _lib.lib().dr_crc32c_extend(init, bytes(data), len(data))


def mask_crc(c):
    return ((((c >> 15) | (c << 17)) & 0xffffffff) + 0xa282ead8) & 0xffffffff


def unmask_crc(m):
    r = (m - 0xa282ead8) & 0xffffffff
    return ((r >> 17) | (r << 15)) & 0xffffffff


# -- protobuf wire encoding (the two messages the bundle index holds) --------
def _varint(v):
    out = bytearray()
    v &= (1 << 64) - 1
    while True:
        b = v & 0x7f
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _read_varint(buf, pos):
    shift = result = 0
    while True:
        b = buf[pos]
        pos += 1
        result |= (b & 0x7f) << shift
        if not b & 0x80:
            return result, pos
        shift += 7


def _field(num, wire, payload):
    return _varint((num << 3) | wire) + payload


def _vfield(num, v):            # proto3 scalar: omitted when 0
    return _field(num, 0, _varint(v)) if v else b""


def _header_proto():
    # BundleHeaderProto {num_shards: 1, endianness: LITTLE (default), version {producer: 1}}
    return _vfield(1, 1) + _field(3, 2, _varint(2) + _vfield(1, 1))


def _entry_proto(dtype, shape, offset, size, crc):
    shp = b"".join(_field(2, 2, _varint(len(d)) + d)
                   for d in (_vfield(1, int(s)) for s in shape))
    return (_vfield(1, dtype) + _field(2, 2, _varint(len(shp)) + shp) + _vfield(4, offset)
            + _vfield(5, size) + _field(6, 5, struct.pack("<I", crc)))


def _parse_entry(buf):
    e = {"dtype": 0, "shape": [], "shard_id": 0, "offset": 0, "size": 0, "crc32c": 0,
         "slices": 0}
    pos = 0
    while pos < len(buf):
        key, pos = _read_varint(buf, pos)
        num, wire = key >> 3, key & 7
        if wire == 0:
            v, pos = _read_varint(buf, pos)
            name = {1: "dtype", 3: "shard_id", 4: "offset", 5: "size", 100: "is_hash_table"}
            if num in name:
                e[name[num]] = v
        elif wire == 5:
            v = struct.unpack_from("<I", buf, pos)[0]
            pos += 4
            if num == 6:
                e["crc32c"] = v
        elif wire == 2:
            n, pos = _read_varint(buf, pos)
            sub = buf[pos:pos + n]
            pos += n
            if num == 2:
                e["shape"] = _parse_shape(sub)
            elif num == 7:
                e["slices"] += 1
        elif wire == 1:
            pos += 8
        else:
            raise _lib.DeepRecError(_lib.INTERNAL, "bad bundle entry wire type %d" % wire)
    return e


def _parse_shape(buf):
    dims, pos = [], 0
    while pos < len(buf):
        key, pos = _read_varint(buf, pos)
        n, pos = _read_varint(buf, pos) if key & 7 == 2 else (0, pos)
        if key >> 3 == 2:
            sub, size, p = buf[pos:pos + n], 0, 0
            while p < len(sub):
                k2, p = _read_varint(sub, p)
                v, p = _read_varint(sub, p) if k2 & 7 == 0 else (0, p)
                if k2 >> 3 == 1:
                    size = v - (1 << 64) if v >= (1 << 63) else v
            dims.append(size)
        elif key >> 3 == 3 and key & 7 == 0:       # unknown_rank
            n = 0
        pos += n
    return dims


# -- SSTable (LevelDB format) -------------------------------------------------
class _Block(object):
    def __init__(self, restart_interval):
        self.ri = restart_interval
        self.buf = bytearray()
        self.restarts = [0]
        self.counter = 0
        self.last = b""

    def add(self, key, value):
        shared = 0
        if self.counter < self.ri:
            m = min(len(key), len(self.last))
            while shared < m and key[shared] == self.last[shared]:
                shared += 1
        else:
            self.restarts.append(len(self.buf))
            self.counter = 0
        self.buf += _varint(shared) + _varint(len(key) - shared) + _varint(len(value))
        self.buf += key[shared:] + value
        self.last = key
        self.counter += 1

    def size_estimate(self):
        return len(self.buf) + 4 * len(self.restarts) + 4

    def finish(self):
        return bytes(self.buf) + b"".join(struct.pack("<I", r) for r in self.restarts) + \
            struct.pack("<I", len(self.restarts))

    def empty(self):
        return not self.buf


def _shortest_separator(start, limit):
    m = min(len(start), len(limit))
    i = 0
    while i < m and start[i] == limit[i]:
        i += 1
    if i < m:
        b = start[i]
        if b < 0xff and b + 1 < limit[i]:
            return start[:i] + bytes([b + 1])
    return start


def _short_successor(key):
    for i, b in enumerate(key):
        if b != 0xff:
            return key[:i] + bytes([b + 1])
    return key


class _TableWriter(object):
    def __init__(self, f, block_size=_BLOCK_SIZE):
        self.f = f
        self.block_size = block_size
        self.offset = 0
        self.data = _Block(_RESTART_INTERVAL)
        self.index = _Block(1)
        self.pending = None            # handle of the last flushed data block
        self.last = b""

    def _write_block(self, contents):
        trailer = b"\x00"
        crc = mask_crc(crc32c(contents + trailer))
        h = (self.offset, len(contents))
        self.f.write(contents + trailer + struct.pack("<I", crc))
        self.offset += len(contents) + 5
        return h

    def add(self, key, value):
        if self.pending is not None:
            self.index.add(_shortest_separator(self.last, key), _varint(self.pending[0]) +
                           _varint(self.pending[1]))
            self.pending = None
        self.data.add(key, value)
        self.last = key
        if self.data.size_estimate() >= self.block_size:
            self._flush()

    def _flush(self):
        if self.data.empty():
            return
        self.pending = self._write_block(self.data.finish())
        self.data = _Block(_RESTART_INTERVAL)

    def finish(self):
        self._flush()
        meta = self._write_block(_Block(_RESTART_INTERVAL).finish())
        if self.pending is not None:
            self.index.add(_short_successor(self.last), _varint(self.pending[0]) +
                           _varint(self.pending[1]))
        idx = self._write_block(self.index.finish())
        footer = _varint(meta[0]) + _varint(meta[1]) + _varint(idx[0]) + _varint(idx[1])
        footer += b"\x00" * (40 - len(footer)) + struct.pack("<Q", _MAGIC)
        self.f.write(footer)


def _read_block(raw, off, size, verify=True):
    contents = raw[off:off + size]
    if verify:
        want = struct.unpack_from("<I", raw, off + size + 1)[0]
        if unmask_crc(want) != crc32c(raw[off:off + size + 1]):
            raise _lib.DeepRecError(_lib.INTERNAL, "corrupted SSTable block at %d" % off)
    n = struct.unpack_from("<I", contents, len(contents) - 4)[0]
    end = len(contents) - 4 - 4 * n
    out, pos, last = [], 0, b""
    while pos < end:
        shared, pos = _read_varint(contents, pos)
        nonshared, pos = _read_varint(contents, pos)
        vlen, pos = _read_varint(contents, pos)
        key = last[:shared] + bytes(contents[pos:pos + nonshared])
        pos += nonshared
        out.append((key, bytes(contents[pos:pos + vlen])))
        pos += vlen
        last = key
    return out


def _read_table(path):
    raw = open(path, "rb").read()
    if len(raw) < 48 or struct.unpack_from("<Q", raw, len(raw) - 8)[0] != _MAGIC:
        raise _lib.DeepRecError(_lib.INTERNAL, "%s is not an SSTable" % path)
    pos = len(raw) - 48
    _, pos = _read_varint(raw, pos)
    _, pos = _read_varint(raw, pos)
    io, pos = _read_varint(raw, pos)
    isz, pos = _read_varint(raw, pos)
    entries = []
    for _, handle in _read_block(raw, io, isz):
        bo, p = _read_varint(handle, 0)
        bs, _ = _read_varint(handle, p)
        entries.extend(_read_block(raw, bo, bs))
    return entries


# -- TensorBundle --------------------------------------------------------------
def data_path(prefix):
    return prefix + ".data-00000-of-00001"


def index_path(prefix):
    return prefix + ".index"


class BundleWriter(object):
    """tensor_bundle.cc BundleWriter: add() appends a tensor's bytes to the
    data file; finish() writes the sorted index."""

    def __init__(self, prefix, block_size=_BLOCK_SIZE):
        self.prefix = prefix
        d = os.path.dirname(prefix)
        if d:
            os.makedirs(d, exist_ok=True)
        self._data = open(data_path(prefix) + ".tmp", "wb")
        self._size = 0
        self._entries = {}
        self._block_size = block_size

    def add(self, key, array):
        key = key.encode() if isinstance(key, str) else bytes(key)
        if not key:
            raise _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, "empty tensor name")
        if key in self._entries:
            raise _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT,
                                            "Adding duplicate key: %s" % key.decode())
        code = None
        if torch.is_tensor(array):
            if array.dtype == torch.bfloat16:
                code = _DT_BFLOAT16
                array = array.detach().contiguous().view(torch.int16)
            array = array.detach().cpu().numpy()
            if code:
                array = array.view(np.uint16)
        a = np.require(array, requirements="C")     # (keeps a rank-0 array rank 0)
        if a.dtype not in _DT:
            raise _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT, "unsupported dtype %s" % a.dtype)
        a = a.astype(a.dtype.newbyteorder("<"), copy=False)
        crc = crc32c(a) if a.nbytes else 0
        self._data.write(memoryview(a).cast("B") if a.nbytes else b"")
        self._entries[key] = _entry_proto(code or _DT[a.dtype], a.shape, self._size, a.nbytes,
                                          mask_crc(crc))
        self._size += a.nbytes

    def finish(self):
        self._data.close()
        os.replace(data_path(self.prefix) + ".tmp", data_path(self.prefix))
        tmp = index_path(self.prefix) + ".tmp"
        with open(tmp, "wb") as f:
            t = _TableWriter(f, self._block_size)
            t.add(b"", _header_proto())
            for k in sorted(self._entries):
                t.add(k, self._entries[k])
            t.finish()
        os.replace(tmp, index_path(self.prefix))


class BundleReader(object):
    """tensor_bundle.cc BundleReader (single shard, little endian)."""

    def __init__(self, prefix):
        self.prefix = prefix
        ents = _read_table(index_path(prefix))
        if not ents or ents[0][0] != b"":
            raise _lib.DeepRecError(_lib.INTERNAL, "bundle index without header")
        self.entries = {k.decode(): _parse_entry(v) for k, v in ents[1:]}
        self._mm = None

    def _data(self):
        if self._mm is None:
            self._mm = np.memmap(data_path(self.prefix), np.uint8, "r") \
                if os.path.getsize(data_path(self.prefix)) else np.zeros(0, np.uint8)
        return self._mm

    def keys(self):
        return sorted(self.entries)

    def contains(self, key):
        return key in self.entries

    def dtype_and_shape(self, key):
        e = self._entry(key)
        return _NP[e["dtype"]], tuple(e["shape"])

    def _entry(self, key):
        if key not in self.entries:
            raise _lib.DeepRecError(_lib.NOT_FOUND, "Key %s not found in checkpoint" % key)
        return self.entries[key]

    def lookup(self, key, verify=True):
        e = self._entry(key)
        dt = _NP[e["dtype"]]
        raw = self._data()[e["offset"]:e["offset"] + e["size"]]
        if verify and e["size"] and unmask_crc(e["crc32c"]) != crc32c(np.asarray(raw)):
            raise _lib.DeepRecError(_lib.INTERNAL, "checksum mismatch for %s" % key)
        return np.frombuffer(raw.tobytes(), dt).reshape(e["shape"]).copy()

    def lookup_rows(self, key, begin, end):
        """Rows [begin, end) of a tensor (LookupSegmentOffset), no checksum."""
        e = self._entry(key)
        dt = _NP[e["dtype"]]
        shape = e["shape"]
        row = int(np.prod(shape[1:], dtype=np.int64)) * dt.itemsize if len(shape) > 1 \
            else dt.itemsize
        raw = self._data()[e["offset"] + begin * row:e["offset"] + end * row]
        return np.frombuffer(raw.tobytes(), dt).reshape((end - begin,) + tuple(shape[1:])).copy()


# -- EmbeddingVariable save / restore ------------------------------------------
def partition_snapshot(keys, values, versions, freqs):
    """DumpEmbeddingValues' layout on the device: keys grouped by key % 1000
    (stable), negative keys dropped.  Returns (offsets int32 [1001], keys,
    values, versions, freqs) as device tensors."""
    from . import ops
    keep = keys >= 0
    if not bool(keep.all()):
        keys, values = keys[keep], values[keep]
        versions = versions[keep] if versions.numel() else versions
        freqs = freqs[keep] if freqs.numel() else freqs
    n = keys.numel()
    offs = torch.zeros(SAVED_PARTITION_NUM + 1, dtype=torch.int32, device=keys.device)
    if n == 0:
        return offs, keys, values, versions, freqs
    ks, perm, counts = ops.partition_by_owner(keys.contiguous(), SAVED_PARTITION_NUM)
    # rows move as their 32-bit words (dr_rows_pack counts a row in floats):
    # a double row is 2 * dim of them, a bf16 row dim / 2
    words = values.contiguous()
    if words.dtype != torch.float32:
        words = words.view(torch.float32)
    vals = torch.empty_like(words)
    ops.rows_pack(words, perm, vals)
    vals = vals.view(values.dtype)
    p64 = perm.to(torch.int64)
    versions = versions[p64] if versions.numel() else versions
    freqs = freqs[p64] if freqs.numel() else freqs
    offs[1:] = torch.cumsum(counts[:SAVED_PARTITION_NUM], 0).to(torch.int32)
    return offs, ks, vals, versions, freqs


def partition_keys(keys):
    """partition_snapshot's rule for a bare key list (a delta's removed
    keys): negative keys dropped, the rest grouped by key % 1000 (stable).
    Returns (offsets int32 [1001], keys) as device tensors."""
    from . import ops
    keys = keys[keys >= 0]
    offs = torch.zeros(SAVED_PARTITION_NUM + 1, dtype=torch.int32, device=keys.device)
    if keys.numel() == 0:
        return offs, keys
    ks, _, counts = ops.partition_by_owner(keys.contiguous(), SAVED_PARTITION_NUM)
    offs[1:] = torch.cumsum(counts[:SAVED_PARTITION_NUM], 0).to(torch.int32)
    return offs, ks


def dump_embedding_values(ev, tensor_key, writer):
    """DumpEmbeddingValues (kv_variable_ops.h:148-265) of one EV (primary or
    slot) under `tensor_key` (e.g. "emb/part_0")."""
    keys, vals, vers, frqs = ev.export()
    offs, keys, vals, vers, frqs = partition_snapshot(keys, vals, vers, frqs)
    write_ev_tensors(writer, tensor_key, offs, keys, vals.reshape(-1, ev.dim), vers, frqs)


def write_ev_tensors(writer, tensor_key, offs, keys, vals, vers, frqs, suffix=""):
    """The five tensors of one EV, in DumpEmbeddingValues' write order
    (partition_offset first, then keys, values, versions, freqs).  `suffix`
    goes between the dash and the tensor's name: "" for a full save,
    INCR_SUFFIX for a delta (NAME-sparse_incr_keys, ...)."""
    pre = tensor_key + "-" + suffix
    writer.add(pre + "partition_offset", offs)
    writer.add(pre + "keys", keys)
    writer.add(pre + "values", vals)
    writer.add(pre + "versions", vers)
    writer.add(pre + "freqs", frqs)


# -- what a checkpoint call accepts beside EVs ---------------------------------
def _kinds():
    from .embedding_ops import DenseSlot, DenseTable, ScalarState
    from .kv_variable_ops import (AdaptiveEmbeddingVariable, EmbeddingVariable,
                                  MultiHashVariable)
    return (EmbeddingVariable, (DenseTable, DenseSlot), ScalarState, MultiHashVariable,
            AdaptiveEmbeddingVariable)


def expand_variables(variables):
    """{tensor_key: object} with the composites replaced by their members, in
    order: a MultiHashVariable under K stands for K/Q and K/R, an
    AdaptiveEmbeddingVariable for K/hash and K/ev.  Everything else -- an
    EmbeddingVariable, a DenseTable, and the DenseSlot / ScalarState objects
    of optimizer.checkpoint_variables -- passes as it is; any other object is
    a TypeError, a tensor key named twice InvalidArgument."""
    ev_t, dense_t, scalar_t, mhv_t, adaptive_t = _kinds()
    out = {}

    def put(key, obj):
        if key in out:
            raise _lib.InvalidArgumentError(_lib.INVALID_ARGUMENT,
                                            "tensor key %s is named twice" % key)
        out[key] = obj
    for key in variables:
        v = variables[key]
        if isinstance(v, mhv_t):
            put(key + "/Q", v.val_list[0])
            put(key + "/R", v.val_list[1])
        elif isinstance(v, adaptive_t):
            put(key + "/hash", v.hash_table)
            put(key + "/ev", v.ev)
        elif isinstance(v, (ev_t, scalar_t)) or isinstance(v, dense_t):
            put(key, v)
        else:
            raise TypeError("checkpoint: %s is %r, not an EmbeddingVariable, a DenseTable, a "
                            "MultiHashVariable, an AdaptiveEmbeddingVariable or an object of "
                            "optimizer.checkpoint_variables" % (key, v))
    return out


def _split_kinds(variables):
    """(expanded dict, its EVs as a dict, its dense objects, its scalars)."""
    ev_t, dense_t, scalar_t = _kinds()[:3]
    allv = expand_variables(variables)
    evs = {k: v for k, v in allv.items() if isinstance(v, ev_t)}
    dense = {k: v for k, v in allv.items() if isinstance(v, dense_t)}
    scalars = {k: v for k, v in allv.items() if isinstance(v, scalar_t)}
    return allv, evs, dense, scalars


def _dense_table(obj):
    """The DenseTable whose update marks a dense object uses."""
    return getattr(obj, "table", obj)


def _scalar_array(s):
    return np.asarray(s.get(), dtype=np.float32).reshape(())


def _check_entry(reader, key, dtype, shape, what):
    """The bundle holds `key` (NOT_FOUND) with this dtype and shape
    (InvalidArgument)."""
    dt, shp = reader.dtype_and_shape(key)
    if reader.entries[key]["dtype"] == _DT_BFLOAT16 or dt != np.dtype(dtype) \
            or tuple(shp) != tuple(shape):
        raise _lib.InvalidArgumentError(
            _lib.INVALID_ARGUMENT, "%s: %s is %s %s in the checkpoint, the variable is %s %s"
            % (what, key, dt, list(shp), np.dtype(dtype), list(shape)))


def _np_dtype(t):
    return np.dtype({torch.float32: np.float32, torch.int64: np.int64,
                     torch.float64: np.float64, torch.int32: np.int32}[t.dtype])


def _put_dense(obj, arr):
    with torch.no_grad():
        obj.weight.copy_(torch.from_numpy(np.ascontiguousarray(arr)))


def save(prefix, variables, global_step=None, compact=False):
    """Saver.save: {tensor_key: variable} -> one bundle.  A variable is an
    EmbeddingVariable (below), a DenseTable -- one entry `tensor_key`,
    [rows, dim] in the table's dtype without slices, as a tf.Variable is
    written -- a MultiHashVariable or AdaptiveEmbeddingVariable (its members,
    expand_variables), or an object of optimizer.checkpoint_variables: a slot
    EV, a dense slot (one entry, like its table) or a scalar (one rank-0
    DT_FLOAT entry).  A dict of EVs alone writes the bytes it always wrote.

    Like DumpEv (save_restore_v2_ops.cc:117-133), each variable's key space
    is shrunk first (EmbeddingVar::Shrink: by L2 weight when the EV has an
    l2_weight_threshold, else by global step when steps_to_live > 0), so
    evicted keys are not written; global_step None skips the step eviction.
    A key space whose primary has a key budget (KeyBudgetEvict, max_keys > 0)
    is then cut down to it (EmbeddingVariable.shrink_to), once, whether or not
    global_step is given.

    compact=True also gives the evicted keys' rows back (EmbeddingVariable.
    compact): each distinct key space once, after its shrink and before its
    first dump.  The bundle's bytes do not depend on it."""
    variables, evs, dense, scalars = _split_kinds(variables)
    w = BundleWriter(prefix)
    compacted = set()
    budgeted = set()
    for name in variables:
        ev = variables[name]
        if name in dense:
            w.add(name, ev.weight)
            continue
        if name in scalars:
            w.add(name, _scalar_array(ev))
            continue
        p = ev._primary or ev
        if p.l2_weight_threshold != -1.0 or (global_step is not None and p.steps_to_live > 0):
            ev.shrink(0 if global_step is None else global_step)
        if p.max_keys > 0 and id(p) not in budgeted:
            budgeted.add(id(p))
            if p.tiered:
                # HBM_DRAM: the keys over the budget go to the host tier, not away, and
                # the dump below (export() merges both tiers) writes them all
                p.demote_to(p.max_keys, p.policy, compact=False)
            else:
                p.shrink_to(p.max_keys, p.policy)
        if compact and id(p) not in compacted:
            compacted.add(id(p))
            p.compact()
        dump_embedding_values(ev, name, w)
    w.finish()
    return prefix


def _part_name(name, part, partition_id):
    i = name.find("part_")
    post = name[i + len("part_") + len(str(partition_id)):]
    return name[:i] + "part_" + str(part) + post


def _import(ev, reader, tname, begin, end, filtered, partition_id, partition_num, suffix="",
            upsert=False):
    tname = tname + "-" + suffix
    keys = reader.lookup_rows(tname + "keys", begin, end)
    n = keys.shape[0]
    if n == 0:
        return
    vals = reader.lookup_rows(tname + "values", begin, end)
    vshape = reader.entries[tname + "versions"]["shape"]
    vers = (reader.lookup_rows(tname + "versions", begin, end) if vshape and vshape[0] > 0
            else np.full(n, -1, np.int64))
    fkey = tname + "freqs"
    if reader.contains(fkey) and reader.entries[fkey]["shape"] and \
            reader.entries[fkey]["shape"][0] > 0:
        frqs = reader.lookup_rows(fkey, begin, end)
    else:
        frqs = np.full(n, ev.filter_freq, np.int64)          # MinFreq
    dev = ev.device
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    if reader.entries[tname + "values"]["dtype"] == _DT_BFLOAT16:
        vals = t(vals.view(np.int16)).view(torch.bfloat16)      # the raw bf16 patterns
    else:
        vals = t(vals)
    if not filtered:
        partition_id = partition_num = 0
    put = ev._upsert if upsert else ev.import_partitioned
    put(t(keys), vals, t(vers), t(frqs), partition_id, partition_num)


def restore_embedding_variable(ev, reader, name, partition_id=0, partition_num=1, suffix="",
                               upsert=False):
    """EVRestoreDynamically (kv_variable_ops.h:459-673).  `suffix` / `upsert`:
    the same walk over a delta's NAME-sparse_incr_* tensors, ending in
    EmbeddingVariable.upsert (restore_incremental)."""
    sfx = "-" + suffix
    if isinstance(reader, str):
        reader = BundleReader(reader)
    if "part_" not in name:                                 # RestoreValue, no filter
        n = reader.dtype_and_shape(name + sfx + "keys")[1][0]
        _import(ev, reader, name, 0, n, False, 0, 1, suffix, upsert)
        return
    new_form = reader.contains(_part_name(name, 0, partition_id) + sfx + "partition_offset")
    part = 0
    while True:
        tname = _part_name(name, part, partition_id)
        if not reader.contains(tname + sfx + "keys"):
            break
        if new_form:
            for key in (sfx + "values", sfx + "versions"):
                # LookupHeader / LookupTensorShape fail on a missing tensor and
                # EVRestoreDynamically treats that as fatal: raise, do not
                # leave the EV half restored
                if not reader.contains(tname + key):
                    raise _lib.DeepRecError(_lib.NOT_FOUND, "Key %s%s not found in checkpoint"
                                       % (tname, key))
            offs = reader.lookup(tname + sfx + "partition_offset")
            for sub in range(partition_id % SAVED_PARTITION_NUM, SAVED_PARTITION_NUM,
                             partition_num):
                if offs[sub + 1] > offs[sub]:
                    _import(ev, reader, tname, int(offs[sub]), int(offs[sub + 1]), True,
                            partition_id, partition_num, suffix, upsert)
        else:                                               # DynamicRestoreValue
            n = reader.dtype_and_shape(tname + sfx + "keys")[1][0]
            _import(ev, reader, tname, 0, n, True, partition_id, partition_num, suffix, upsert)
        part += 1


def restore(prefix, variables, partition_id=0, partition_num=1):
    """Restore {tensor_key: variable} (the kinds save() takes) from a bundle.
    A key space with a host-DRAM tier (StorageType.HBM_DRAM) ends within its
    HBM budget: once all its variables are in, the keys over it are demoted.
    A dense table, dense slot or scalar whose entry is missing is NOT_FOUND,
    one whose entry has another shape or dtype InvalidArgument; both (and an
    unpartitioned EV name without its -keys tensor) are raised before any
    variable of the call has been changed."""
    variables, evs, dense, scalars = _split_kinds(variables)
    r = BundleReader(prefix)
    # every refusal first: nothing is changed by a call that raises one
    for name, obj in dense.items():
        _check_entry(r, name, _np_dtype(obj.weight), obj.weight.shape, "restore")
    for name in scalars:
        _check_entry(r, name, np.float32, (), "restore")
    for name in evs:
        if "part_" not in name:
            r.dtype_and_shape(name + "-keys")
    for name in variables:
        if name in dense:
            _put_dense(variables[name], r.lookup(name))
        elif name in scalars:
            variables[name].set(float(r.lookup(name)))
        else:
            restore_embedding_variable(variables[name], r, name, partition_id, partition_num)
    tiered = {id(ev._primary or ev): (ev._primary or ev) for ev in evs.values()
              if ev.tiered}
    for p in tiered.values():
        p.demote_to()


# -- incremental checkpoints (build-defined) ----------------
INCR_SUFFIX = "sparse_incr_"


def save_incremental(prefix, variables, global_step=None):
    """IncrSave's role: one bundle with, for every named EV (primaries and
    slots), NAME-sparse_incr_{partition_offset, keys, values, versions,
    freqs} holding the keys marked as updated since the key space was last
    cleared (EmbeddingVariable.export_updated), in the full save's layout:
    grouped by key % 1000, negative keys dropped, versions / freqs empty when
    the EV keeps none.  Every key space must be tracking (track_updates()).
    Each distinct key space is cleared once, after all of its columns are
    written.

    Evictions: with `global_step` given, a key space whose primary has
    steps_to_live > 0 or an l2_weight_threshold is shrunk first, exactly as
    save() does (global_step None shrinks nothing: eviction then stays with
    the full save).  A key budget is different: a key space whose primary
    has one (KeyBudgetEvict, max_keys > 0) is cut down to it
    (EmbeddingVariable.shrink_to) whether or not global_step is given, after
    that shrink -- the budget bounds the table, and a trainer that only writes
    deltas must stay inside it too.  A key space that logs removals (track_removals()) also
    gets, under its PRIMARY's tensor key and after that name's five tensors,
    NAME-sparse_incr_removed_partition_offset (int32 [1001]) and
    NAME-sparse_incr_removed_keys: the distinct keys shrink() / remove() /
    shrink_to() dropped since the log was last cleared, negative keys dropped and the
    rest grouped by key % 1000; the log is cleared with the marks.  The
    primary of such a key space must be among `variables`.  A key space that
    does not log removals gets neither tensor and its delta carries no
    evictions: an evicted key is simply absent from it, and a replica drops
    it at its next full restore.  A key space with a host-DRAM tier is
    refused before anything is shrunk, as its track_updates() is, unless it
    opted in (StorageOption(StorageType.HBM_DRAM, incremental=True); DESIGN
    section 17).  Then the age rule runs on both tiers, the keys over the
    budget are demoted (demote_to, compact=False: they stay in the model and
    out of the removal log) in place of shrink_to, and the delta holds the
    marked keys of both tiers -- the bytes an untiered, unbudgeted trainer
    that saw the same calls writes.

    Beside EVs the call takes what save() takes.  A dense table or dense slot
    writes NAME-sparse_incr_keys (int64 [m], the marked row ids ascending) and
    NAME-sparse_incr_values ([m, dim]; int64 [m] for AdagradDecay's count); a
    table that is not tracking (DenseTable.track_updates()) is refused by
    name before anything is shrunk or written, and each table's marks are
    cleared once, after all of its columns are written.  A scalar is written
    whole under its own key.  Returns `prefix`."""
    allv, variables, dense, scalars = _split_kinds(variables)
    for ev in variables.values():
        ev._refuse_tiered("save_incremental")
    tables = {}
    for name, obj in dense.items():
        t = _dense_table(obj)
        if not t.tracking_updates():
            raise _lib.InvalidArgumentError(
                _lib.INVALID_ARGUMENT, "save_incremental: dense table %s is not tracking "
                "updates (track_updates())" % (t.name or name))
        tables[id(t)] = t
    w = BundleWriter(prefix)
    spaces = {}
    for ev in variables.values():
        p = ev._primary or ev
        if id(p) in spaces:
            continue
        spaces[id(p)] = p
        if p.tracking_removals() and not any(v is p for v in variables.values()):
            raise _lib.InvalidArgumentError(
                _lib.INVALID_ARGUMENT, "save_incremental: %s logs removals, which are written "
                "under the primary's tensor key: name it in `variables`" % p.name)
        if global_step is not None and (p.l2_weight_threshold != -1.0 or p.steps_to_live > 0):
            p.shrink(global_step)
        if p.max_keys > 0:
            if p.tiered:
                # HBM_DRAM (opted in): the keys over the budget go to the host tier with
                # their update bits, not away; export_updated() below merges both tiers
                p.demote_to(p.max_keys, p.policy, compact=False)
            else:
                p.shrink_to(p.max_keys, p.policy)
    for name in allv:
        if name in dense:
            rows, vals = dense[name].export_updated()
            w.add(name + "-" + INCR_SUFFIX + "keys", rows)
            w.add(name + "-" + INCR_SUFFIX + "values", vals)
            continue
        if name in scalars:
            w.add(name, _scalar_array(scalars[name]))
            continue
        ev = variables[name]
        keys, vals, vers, frqs = ev.export_updated()
        offs, keys, vals, vers, frqs = partition_snapshot(keys, vals, vers, frqs)
        write_ev_tensors(w, name, offs, keys, vals.reshape(-1, ev.dim), vers, frqs, INCR_SUFFIX)
        if ev._primary is None and ev.tracking_removals():
            offs, keys = partition_keys(ev.export_removed())
            w.add(name + "-" + INCR_SUFFIX + "removed_partition_offset", offs)
            w.add(name + "-" + INCR_SUFFIX + "removed_keys", keys)
    w.finish()
    for p in spaces.values():
        p.clear_updated()
        if p.tracking_removals():
            p.clear_removed()
    for t in tables.values():
        t.clear_updated()
    return prefix


def restore_incremental(prefix, variables, partition_id=0, partition_num=1, compact=False):
    """KvResourceIncrImport's role: apply a delta written by save_incremental
    to {tensor_key: EmbeddingVariable}, in two passes.  First the delta's
    removals: for every primary whose name has NAME-sparse_incr_removed_keys
    in the bundle (every saved part of a partitioned name), remove() those
    keys, once per key space and without a partition filter -- absent keys
    are ignored.  Then the walk of restore() (parts, sub-partitions, the
    key % 1000 % partition_num filter) over the NAME-sparse_incr_* tensors,
    ending in upsert: rows of keys already present are overwritten, new keys
    are created.  Removals first, upserts second: a key that was evicted,
    re-created and updated again ends with its new row, and one that was
    re-created but never updated ends absent, so the replica serves the
    default as the trainer's fresh row does.  compact=True compacts each
    distinct key space once at the end (EmbeddingVariable.compact), which is
    what keeps a replica fed by deltas alone bounded.  A delta without the
    removed_* tensors restores as before.  A key space with a host-DRAM tier
    is refused, as its track_updates() is, unless it opted in
    (StorageOption(StorageType.HBM_DRAM, incremental=True)): then the removals
    reach both tiers, an upsert promotes its keys first, and the key space
    ends within its HBM budget (demote_to), as restore() ends.  A dense table
    or dense slot takes its NAME-sparse_incr_{keys, values} through upsert
    (dr_dense_upsert_rows) and a scalar its whole value; their missing or
    mis-shaped entries are raised before anything is changed."""
    allv, variables, dense, scalars = _split_kinds(variables)
    for ev in variables.values():
        ev._refuse_tiered("restore_incremental")
    r = BundleReader(prefix)
    # the dense objects' and scalars' refusals first, as restore() does
    for name, obj in dense.items():
        kname, vname = (name + "-" + INCR_SUFFIX + s for s in ("keys", "values"))
        m = r.dtype_and_shape(kname)[1]
        _check_entry(r, kname, np.int64, m, "restore_incremental")
        _check_entry(r, vname, _np_dtype(obj.weight), tuple(m) + tuple(obj.weight.shape[1:]),
                     "restore_incremental")
    for name in scalars:
        _check_entry(r, name, np.float32, (), "restore_incremental")
    for name, obj in dense.items():
        rows = r.lookup(name + "-" + INCR_SUFFIX + "keys")
        if rows.size:
            dev = obj.weight.device
            obj.upsert(torch.as_tensor(rows, device=dev),
                       torch.as_tensor(r.lookup(name + "-" + INCR_SUFFIX + "values"), device=dev))
    for name, s in scalars.items():
        s.set(float(r.lookup(name)))
    sfx = "-" + INCR_SUFFIX + "removed_keys"
    for name in variables:
        ev = variables[name]
        if ev._primary is not None:
            continue
        if "part_" not in name:
            tnames = [name]
        else:
            tnames, part = [], 0
            while r.contains(_part_name(name, part, partition_id) + "-" + INCR_SUFFIX + "keys"):
                tnames.append(_part_name(name, part, partition_id))
                part += 1
        gone = [r.lookup(t + sfx) for t in tnames if r.contains(t + sfx)]
        gone = [g for g in gone if g.size]
        if gone:
            ev.remove(torch.as_tensor(np.concatenate(gone), device=ev.device))
    for name in variables:
        restore_embedding_variable(variables[name], r, name, partition_id, partition_num,
                                   INCR_SUFFIX, True)
    if compact:
        done = set()
        for ev in variables.values():
            p = ev._primary or ev
            if id(p) not in done:
                done.add(id(p))
                p.compact()
    # as restore() ends: a tiered key space is back within its HBM budget
    tiered = {id(ev._primary or ev): (ev._primary or ev) for ev in variables.values()
              if ev.tiered}
    for p in tiered.values():
        p.demote_to()
