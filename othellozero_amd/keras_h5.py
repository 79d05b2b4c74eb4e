"""Keras HDF5 weight files without h5py -- SURVEY.md section 8(f) item 1 (weights interchange).

The reference saves / loads checkpoints with `model.save_weights(path, save_format='h5')` / `model.load_weights(path)`
(Net/NNet.py:90-96; workers.py ships these files to remote workers, main.py:138-150 keeps `*-best.h5` files).  Neither
h5py nor TensorFlow exists in this image, so this module restates, from the published HDF5 File Format Specification
(version 3.0) and Keras 2.4 `hdf5_format.py` (tensorflow==2.3.1, requirements.txt), exactly the subset those calls touch:

reader  superblock v0/v1 (what h5py's default libver writes) and v2/v3; object headers v1 and v2 with continuation
        blocks; old-style groups (symbol-table message -> v1 B-tree -> SNOD -> local heap) and compact new-style groups
        (link messages); dataspace v1/v2; fixed / float / fixed-string / variable-length-string datatypes (global heap);
        attribute messages v1-v3; contiguous and compact dataset layouts.  Chunked / filtered datasets and dense
        (fractal-heap) link or attribute storage are rejected loudly -- Keras weight files never contain them.
writer  superblock v0, v1 object headers, symbol-table groups, fixed-length string attributes, contiguous float32
        datasets: the same structures libhdf5 1.10 emits for Keras, so h5py / Keras read the files back.

Pinned by tests/golden/keras_weights_*.h5 (made by the genuine libhdf5 1.10.6 with h5py's call sequence,
tests/golden/gen_keras_h5.py) and by reading this writer's output back through the genuine library (tests/test_keras_h5.py).
Host-side file I/O only; no GPU involvement.
"""
import struct

import numpy as np

UNDEF = 0xFFFFFFFFFFFFFFFF
SIGNATURE = b"\x89HDF\r\n\x1a\n"
HDF5_OBJECT_HEADER_LIMIT = 64512          # keras hdf5_format.py


class H5FormatError(Exception):
    pass


# =====================================================================================================================
# reader
# =====================================================================================================================
class _Dtype:
    def __init__(self, kind, size, np_dtype=None, base=None, vlen_string=False):
        self.kind, self.size, self.np_dtype, self.base, self.vlen_string = kind, size, np_dtype, base, vlen_string


class H5Object:
    """a group or a dataset: .attrs (dict), .links (name -> address, groups), dataset fields"""

    def __init__(self, f, addr):
        self.file, self.addr = f, addr
        self.attrs, self.links = {}, None
        self.dtype = self.shape = self.layout = None
        self._symtab = None

    @property
    def is_dataset(self):
        return self.layout is not None

    def keys(self):
        return list(self._children())

    def _children(self):
        if self.links is None:
            self.links = {}
            if self._symtab is not None:
                self.file._walk_btree(self._symtab[0], self._symtab[1], self.links)
        return self.links

    def __contains__(self, name):
        try:
            self[name]
            return True
        except KeyError:
            return False

    def __getitem__(self, path):
        obj = self
        for part in [p for p in path.split("/") if p]:
            ch = obj._children()
            if part not in ch:
                raise KeyError(path)
            obj = self.file._object(ch[part])
        return obj

    def read(self):
        """dataset -> ndarray"""
        if not self.is_dataset:
            raise H5FormatError("not a dataset")
        count = int(np.prod(self.shape, dtype=np.int64)) if self.shape else 1
        kind = self.layout[0]
        if kind == "contiguous":
            _, addr, size = self.layout
            raw = b"" if addr == UNDEF else self.file._bytes(addr, count * self.dtype.size)
            if addr == UNDEF:                       # never written: fill value (zeros)
                raw = bytes(count * self.dtype.size)
        elif kind == "compact":
            raw = self.layout[1][:count * self.dtype.size]
        else:
            raise H5FormatError(f"dataset layout '{kind}' is not supported (Keras weight files are contiguous)")
        return self.file._decode(raw, self.dtype, self.shape)


class H5File(H5Object):
    """Read-only view of an HDF5 file (the subset listed in the module docstring)."""

    def __init__(self, path):
        with open(path, "rb") as fh:
            self.buf = fh.read()
        self._cache = {}
        base = self._find_superblock()
        ver = self.buf[base + 8]
        if ver in (0, 1):
            self.O, self.L = self.buf[base + 13], self.buf[base + 14]
            p = base + 24 + (4 if ver == 1 else 0)
            self.base_addr = self._uint(p, self.O)
            p += 4 * self.O                                   # base, free-space info, end of file, driver info
            root_addr = self._uint(p + self.O, self.O)        # symbol table entry: link name offset, object header address
        elif ver in (2, 3):
            self.O, self.L = self.buf[base + 9], self.buf[base + 10]
            self.base_addr = self._uint(base + 12, self.O)
            root_addr = self._uint(base + 12 + 3 * self.O, self.O)
        else:
            raise H5FormatError(f"superblock version {ver} is not supported")
        if self.O != 8 or self.L != 8:
            raise H5FormatError("only 8-byte offsets / lengths are supported")
        H5Object.__init__(self, self, root_addr)
        self._parse_header(self)
        self._cache[root_addr] = self

    # ---- low level
    def _find_superblock(self):
        off = 0
        while off + 8 <= len(self.buf):
            if self.buf[off:off + 8] == SIGNATURE:
                return off
            off = 512 if off == 0 else off * 2
        raise H5FormatError("not an HDF5 file (signature not found)")

    def _bytes(self, addr, n):
        a = addr + self.base_addr
        if a < 0 or a + n > len(self.buf):
            raise H5FormatError("address outside the file (truncated file?)")
        return self.buf[a:a + n]

    def _uint(self, pos, n):
        return int.from_bytes(self.buf[pos:pos + n], "little")

    def _object(self, addr):
        if addr not in self._cache:
            o = H5Object(self, addr)
            self._parse_header(o)
            self._cache[addr] = o
        return self._cache[addr]

    # ---- object headers
    def _parse_header(self, obj):
        a = obj.addr + self.base_addr
        if self.buf[a:a + 4] == b"OHDR":
            msgs = self._messages_v2(a)
        elif self.buf[a] == 1:
            msgs = self._messages_v1(a)
        else:
            raise H5FormatError(f"unknown object header at {obj.addr:#x}")
        links = {}
        for mtype, data in msgs:
            if mtype == 0x0001:
                obj.shape = self._dataspace(data)
            elif mtype == 0x0003:
                obj.dtype = self._datatype(data)[0]
            elif mtype == 0x0008:
                obj.layout = self._layout(data)
            elif mtype == 0x000C:
                name, value = self._attribute(data)
                obj.attrs[name] = value
            elif mtype == 0x0011:
                obj._symtab = (int.from_bytes(data[0:8], "little"), int.from_bytes(data[8:16], "little"))
            elif mtype == 0x0006:
                name, addr = self._link(data)
                if addr is not None:
                    links[name] = addr
            elif mtype == 0x0002:
                self._link_info(data)
            elif mtype == 0x0015:
                self._attr_info(data)
            elif mtype == 0x000B:
                raise H5FormatError("filtered (compressed) datasets are not supported")
        if links or (obj._symtab is None and obj.layout is None):
            obj.links = links

    def _messages_v1(self, a):
        nmsg = self._uint(a + 2, 2)
        size = self._uint(a + 8, 4)
        blocks, out = [(a + 16, size)], []
        while blocks and len(out) < nmsg:
            p, n = blocks.pop(0)
            end = p + n
            while p + 8 <= end and len(out) < nmsg:
                mtype, msize = self._uint(p, 2), self._uint(p + 2, 2)
                data = self.buf[p + 8:p + 8 + msize]
                p += 8 + msize
                if mtype == 0x0010:
                    blocks.append((int.from_bytes(data[0:8], "little") + self.base_addr, int.from_bytes(data[8:16], "little")))
                out.append((mtype, data))
        return out

    def _messages_v2(self, a):
        flags = self.buf[a + 5]
        p = a + 6
        if flags & 0x20:
            p += 16
        if flags & 0x10:
            p += 4
        w = 1 << (flags & 3)
        size = self._uint(p, w)
        p += w
        blocks, out = [(p, size)], []
        while blocks:
            p, n = blocks.pop(0)
            end = p + n
            hdr = 4 + (2 if flags & 0x04 else 0)
            while p + hdr <= end:
                mtype, msize = self.buf[p], self._uint(p + 1, 2)
                data = self.buf[p + hdr:p + hdr + msize]
                p += hdr + msize
                if mtype == 0x10:
                    ca, cl = int.from_bytes(data[0:8], "little") + self.base_addr, int.from_bytes(data[8:16], "little")
                    if self.buf[ca:ca + 4] != b"OCHK":
                        raise H5FormatError("bad object header continuation block")
                    blocks.append((ca + 4, cl - 8))          # minus signature and checksum
                elif mtype != 0:
                    out.append((mtype, data))
        return out

    # ---- messages
    def _dataspace(self, d):
        ver, rank, flags = d[0], d[1], d[2]
        if ver == 1:
            p = 8
        elif ver == 2:
            if d[3] == 2:                                   # null dataspace
                return (0,)
            p = 4
        else:
            raise H5FormatError(f"dataspace message version {ver}")
        return tuple(int.from_bytes(d[p + 8 * i:p + 8 * i + 8], "little") for i in range(rank))

    def _datatype(self, d):
        """-> (_Dtype, bytes consumed)"""
        cls, ver = d[0] & 0x0F, d[0] >> 4
        b0, b1 = d[1], d[2]
        size = int.from_bytes(d[4:8], "little")
        order = ">" if b0 & 1 else "<"
        if cls == 0:
            return _Dtype("int", size, np.dtype(f"{order}{'i' if b0 & 8 else 'u'}{size}")), 12
        if cls == 1:
            if size not in (2, 4, 8):
                raise H5FormatError(f"float of {size} bytes")
            return _Dtype("float", size, np.dtype(f"{order}f{size}")), 20
        if cls == 3:
            return _Dtype("string", size, np.dtype(f"S{size}")), 8
        if cls == 9:
            base, used = self._datatype(d[8:])
            return _Dtype("vlen", size, base=base, vlen_string=(b0 & 0x0F) == 1), 8 + used
        raise H5FormatError(f"datatype class {cls} is not supported")

    def _layout(self, d):
        ver = d[0]
        if ver in (3, 4):
            cls = d[1]
            if cls == 0:
                n = int.from_bytes(d[2:4], "little")
                return ("compact", bytes(d[4:4 + n]))
            if cls == 1:
                return ("contiguous", int.from_bytes(d[2:10], "little"), int.from_bytes(d[10:18], "little"))
            return ("chunked",)
        if ver in (1, 2):
            rank, cls = d[1], d[2]
            if cls == 1:
                return ("contiguous", int.from_bytes(d[8:16], "little"), None)
            return ("chunked",) if cls == 2 else ("compact", bytes(d[8 + 4 * rank + 4:]))
        raise H5FormatError(f"data layout message version {ver}")

    def _attribute(self, d):
        ver = d[0]
        nsz, tsz, ssz = (int.from_bytes(d[2 + 2 * i:4 + 2 * i], "little") for i in range(3))
        if ver == 1:
            pad = lambda x: (x + 7) & ~7
            p = 8
        elif ver in (2, 3):
            if d[1] & 3:
                raise H5FormatError("shared attribute datatypes / dataspaces are not supported")
            pad = lambda x: x
            p = 8 if ver == 2 else 9
        else:
            raise H5FormatError(f"attribute message version {ver}")
        name = bytes(d[p:p + nsz]).split(b"\0")[0].decode("utf8")
        p += pad(nsz)
        dt = self._datatype(d[p:p + tsz])[0]
        p += pad(tsz)
        shape = self._dataspace(d[p:p + ssz]) if ssz else ()
        p += pad(ssz)
        return name, self._decode(bytes(d[p:]), dt, shape)

    def _link(self, d):
        flags = d[1]
        p = 2
        ltype = 0
        if flags & 0x08:
            ltype = d[p]
            p += 1
        if flags & 0x04:
            p += 8
        if flags & 0x10:
            p += 1
        w = 1 << (flags & 3)
        n = int.from_bytes(d[p:p + w], "little")
        p += w
        name = bytes(d[p:p + n]).decode("utf8")
        p += n
        return name, (int.from_bytes(d[p:p + 8], "little") if ltype == 0 else None)

    def _link_info(self, d):
        p = 2 + (8 if d[1] & 1 else 0)
        if int.from_bytes(d[p:p + 8], "little") != UNDEF:
            raise H5FormatError("dense (fractal heap) group storage is not supported")

    def _attr_info(self, d):
        p = 2 + (2 if d[1] & 1 else 0)
        if int.from_bytes(d[p:p + 8], "little") != UNDEF:
            raise H5FormatError("dense (fractal heap) attribute storage is not supported")

    # ---- old-style groups
    def _walk_btree(self, btree, heap, out):
        hb = self._bytes(heap, 32)
        if hb[:4] != b"HEAP":
            raise H5FormatError("bad local heap")
        hsize, hdata = int.from_bytes(hb[8:16], "little"), int.from_bytes(hb[24:32], "little")
        names = self._bytes(hdata, hsize)

        def node(addr):
            b = self._bytes(addr, 24)
            if b[:4] == b"SNOD":
                count = int.from_bytes(b[6:8], "little")
                ent = self._bytes(addr + 8, 40 * count)
                for i in range(count):
                    noff = int.from_bytes(ent[40 * i:40 * i + 8], "little")
                    oaddr = int.from_bytes(ent[40 * i + 8:40 * i + 16], "little")
                    end = names.index(b"\0", noff)
                    out[names[noff:end].decode("utf8")] = oaddr
                return
            if b[:4] != b"TREE" or b[4] != 0:
                raise H5FormatError("bad group B-tree node")
            used = int.from_bytes(b[6:8], "little")
            body = self._bytes(addr + 24, 16 * used + 8)
            for i in range(used):
                node(int.from_bytes(body[16 * i + 8:16 * i + 16], "little"))
        node(btree)

    # ---- data decoding
    def _decode(self, raw, dt, shape):
        count = int(np.prod(shape, dtype=np.int64)) if shape else 1
        if dt.kind == "vlen":
            if not dt.vlen_string:
                raise H5FormatError("variable-length sequences are not supported")
            vals = []
            for i in range(count):
                e = raw[16 * i:16 * i + 16]
                vals.append(self._global_heap_object(int.from_bytes(e[4:12], "little"), int.from_bytes(e[12:16], "little"))
                            [:int.from_bytes(e[0:4], "little")])
            arr = np.array(vals, dtype=object).reshape(shape) if shape else vals[0]
            return arr
        arr = np.frombuffer(raw[:count * dt.size], dtype=dt.np_dtype, count=count)
        return arr.reshape(shape).copy() if shape else arr[0]

    def _global_heap_object(self, addr, index):
        b = self._bytes(addr, 16)
        if b[:4] != b"GCOL":
            raise H5FormatError("bad global heap collection")
        size = int.from_bytes(b[8:16], "little")
        col = self._bytes(addr, size)
        p = 16
        while p + 16 <= size:
            idx, n = int.from_bytes(col[p:p + 2], "little"), int.from_bytes(col[p + 8:p + 16], "little")
            if idx == index:
                return bytes(col[p + 16:p + 16 + n])
            if idx == 0:
                break
            p += 16 + ((n + 7) & ~7)
        raise H5FormatError("global heap object not found")


# =====================================================================================================================
# writer
# =====================================================================================================================
GROUP_LEAF_K, GROUP_INTERNAL_K = 4, 16            # libhdf5 defaults: 8 symbols per SNOD, 32 SNODs per B-tree node


def _pad8(b):
    return b + bytes(-len(b) % 8)


def _msg(mtype, data, flags=0):
    data = _pad8(data)
    return struct.pack("<HHB3x", mtype, len(data), flags) + data


def _dataspace_msg(shape):
    """v1; like H5Screate_simple(rank, dims, NULL): maximum dims present and equal to dims"""
    dims = b"".join(struct.pack("<Q", s) for s in shape)
    return struct.pack("<BBB5x", 1, len(shape), 1 if shape else 0) + dims + dims


_F32_TYPE = struct.pack("<BBBBI", 0x11, 0x20, 0x1F, 0x00, 4) + struct.pack("<HHBBBBI", 0, 32, 23, 8, 0, 23, 127)
_F64_TYPE = struct.pack("<BBBBI", 0x11, 0x20, 0x3F, 0x00, 8) + struct.pack("<HHBBBBI", 0, 64, 52, 11, 0, 52, 1023)


def _string_type(size):
    return struct.pack("<BBBBI", 0x13, 0x01, 0x00, 0x00, size)      # class 3 v1, null-padded, ASCII


def _attr_msg(name, value):
    """value: bytes (scalar fixed string), list/array of bytes (1-D fixed strings), or an empty list (float64, dims (0,))"""
    arr = np.asarray(value)
    if arr.size == 0:
        dt, shape, raw = _F64_TYPE, (0,), b""
    elif arr.dtype.kind == "S":
        dt, shape, raw = _string_type(arr.dtype.itemsize), arr.shape, np.ascontiguousarray(arr).tobytes()
    else:
        raise TypeError("only byte-string attributes are written")
    nm = name.encode("utf8") + b"\0"
    ds = _dataspace_msg(shape)
    body = struct.pack("<BxHHH", 1, len(nm), len(dt), len(ds)) + _pad8(nm) + _pad8(dt) + _pad8(ds) + raw
    if len(body) > 0xFFF8:
        raise H5FormatError(f"attribute '{name}' does not fit an object header message")
    return _msg(0x000C, body)


class _Writer:
    def __init__(self):
        self.buf = bytearray()

    def alloc(self, n):
        self.buf += bytes(-len(self.buf) % 8)
        a = len(self.buf)
        self.buf += bytes(n)
        return a

    def put(self, addr, data):
        self.buf[addr:addr + len(data)] = data

    def object_header(self, messages):
        body = b"".join(messages)
        a = self.alloc(16 + len(body))
        self.put(a, struct.pack("<BxHII4x", 1, len(messages), 1, len(body)) + body)
        return a

    def dataset(self, arr):
        arr = np.asarray(arr, dtype="<f4")              # 0-d stays 0-d (a scalar dataspace, like h5py's dset[()] = val)
        raw = arr.tobytes(order="C")
        daddr = self.alloc(len(raw)) if raw else UNDEF
        if raw:
            self.put(daddr, raw)
        msgs = [_msg(0x0001, _dataspace_msg(arr.shape)),
                _msg(0x0003, _F32_TYPE, flags=1),                                 # constant message, like libhdf5
                _msg(0x0005, struct.pack("<BBBBI", 2, 2, 2, 1, 0)),               # fill value v2: late alloc, write if set, default value
                _msg(0x0008, struct.pack("<BBQQ", 3, 1, daddr, len(raw)))]
        return self.object_header(msgs)

    def group(self, children, attr_msgs=()):
        """children: {name: object header address}.  Returns (header address, btree address, heap address)."""
        names = sorted(children, key=lambda s: s.encode("utf8"))
        heap = bytearray(8)                                                      # offset 0: the empty name
        offs = {}
        for nme in names:
            offs[nme] = len(heap)
            heap += _pad8(nme.encode("utf8") + b"\0")
        hdata = self.alloc(max(len(heap), 8))
        self.put(hdata, bytes(heap))
        haddr = self.alloc(32)
        self.put(haddr, b"HEAP" + struct.pack("<B3xQQQ", 0, len(heap), 1, hdata))   # free-list head 1 = none
        per = 2 * GROUP_LEAF_K
        leaves = [names[i:i + per] for i in range(0, len(names), per)] or [[]]
        if len(leaves) > 2 * GROUP_INTERNAL_K:
            raise H5FormatError("too many links in one group for a single-level B-tree")
        snods = []
        for leaf in leaves:
            sa = self.alloc(8 + per * 40)
            ent = b"".join(struct.pack("<QQII16x", offs[nme], children[nme], 0, 0) for nme in leaf)
            self.put(sa, b"SNOD" + struct.pack("<BxH", 1, len(leaf)) + ent)
            snods.append(sa)
        baddr = self.alloc(24 + 2 * GROUP_INTERNAL_K * 8 + (2 * GROUP_INTERNAL_K + 1) * 8)
        used = len(leaves) if names else 0
        body = struct.pack("<Q", 0)
        for leaf, sa in zip(leaves[:used], snods):
            body += struct.pack("<QQ", sa, offs[leaf[-1]])
        self.put(baddr, b"TREE" + struct.pack("<BBHQQ", 0, 0, used, UNDEF, UNDEF) + body)
        hdr = self.object_header([_msg(0x0011, struct.pack("<QQ", baddr, haddr))] + list(attr_msgs))
        return hdr, baddr, haddr


def _split_attr(name, values):
    """keras save_attributes_to_hdf5_group: split a long name list over name0, name1, ... (64512-byte header limit)"""
    data = np.asarray(values)
    if data.size == 0:
        return [(name, [])]
    chunks, n = [data], 1
    while any(c.nbytes > HDF5_OBJECT_HEADER_LIMIT for c in chunks):
        n += 1
        chunks = np.array_split(data, n)
    return [(name, data)] if n == 1 else [(f"{name}{i}", c) for i, c in enumerate(chunks)]


def write_h5(path, root_attrs, groups):
    """Generic Keras-style writer.  root_attrs: [(name, bytes | [bytes])]; groups: [(group name, attrs, [(dataset path
    relative to the group, ndarray)])] -- dataset paths may contain '/', intermediate groups are created."""
    w = _Writer()
    w.alloc(96)                                                                  # superblock v0 (8-byte offsets)

    def build(tree, attrs):
        kids = {}
        for nme, sub in tree.items():
            kids[nme] = w.dataset(sub) if isinstance(sub, np.ndarray) else build(sub[0], sub[1])[0]
        msgs = [_attr_msg(k, v) for k, v in attrs]
        return w.group(kids, msgs)

    tree = {}
    for gname, gattrs, dsets in groups:
        sub = {}
        for dpath, arr in dsets:
            parts = [p for p in dpath.split("/") if p]
            cur = sub
            for p in parts[:-1]:
                cur = cur.setdefault(p, ({}, []))[0]
            cur[parts[-1]] = np.asarray(arr)
        if gname in tree:
            raise H5FormatError(f"duplicate layer name '{gname}'")
        tree[gname] = (sub, list(gattrs))
    root, rb, rh = build(tree, root_attrs)
    eof = len(w.buf) + (-len(w.buf) % 8)
    w.buf += bytes(eof - len(w.buf))
    sb = SIGNATURE + struct.pack("<BBBBBBBBHHI", 0, 0, 0, 0, 0, 8, 8, 0, GROUP_LEAF_K, GROUP_INTERNAL_K, 0)
    sb += struct.pack("<QQQQ", 0, UNDEF, eof, UNDEF)
    sb += struct.pack("<QQII", 0, root, 1, 0) + struct.pack("<QQ", rb, rh)       # root symbol-table entry, cached
    assert len(sb) == 96
    w.put(0, sb)
    with open(path, "wb") as fh:
        fh.write(bytes(w.buf))


# =====================================================================================================================
# Keras weight-file layer on top
# =====================================================================================================================
AUX_LAYERS = ("ownership", "score")     # the two Dense layers of the trainer's auxiliary heads, behind `v` in a file that carries them


def keras_layer_table(weights, model_index=0, network="ONN", aux=None):
    """The `model.layers` of OthelloNN / BaseNN (Net/OthelloNN.py:42-54, Net/BaseNN.py:41-54) with Keras' automatic
    names, for the `model_index`-th such model built in a process (the reference builds several: main.py:275-300),
    paired with the 40 get_weights() arrays.  -> [(layer name, [(weight name, array)])], weightless layers included.
    BaseNN has an unnamed Reshape after the input and another after `pi` where OthelloNN has `pi-reshaped`.
    aux: None or the four arrays of the auxiliary heads (Wown, bown, Wsc, bsc): two more Dense layers, `ownership` and `score`, at the end."""
    assert len(weights) == 40, "expected the 40 arrays of get_weights()"
    m = model_index
    sfx = lambda base, k: base if k == 0 else f"{base}_{k}"
    bn_names = ("gamma:0", "beta:0", "moving_mean:0", "moving_variance:0")
    layers = [(f"input_{m + 1}", [])] + ([(sfx("reshape", 2 * m), [])] if network == "BNN" else [])
    it = iter(weights)
    take = lambda lname, wnames: (lname, [(f"{lname}/{wn}", np.asarray(next(it), dtype=np.float32)) for wn in wnames])
    for i in range(4):
        layers += [take(sfx("conv2d", 4 * m + i), ("kernel:0", "bias:0")),
                   take(sfx("batch_normalization", 6 * m + i), bn_names), (sfx("activation", 6 * m + i), [])]
    layers.append((sfx("flatten", m), []))
    for i in range(2):
        layers += [take(sfx("dense", 2 * m + i), ("kernel:0", "bias:0")),
                   take(sfx("batch_normalization", 6 * m + 4 + i), bn_names), (sfx("activation", 6 * m + 4 + i), []),
                   (sfx("dropout", 2 * m + i), [])]
    layers += [take("pi", ("kernel:0", "bias:0")), (sfx("reshape", 2 * m + 1) if network == "BNN" else "pi-reshaped", []),
               take("v", ("kernel:0", "bias:0"))]
    if aux is not None:
        assert len(aux) == 4, "expected the four arrays of the auxiliary heads"
        it = iter(aux)
        layers += [take(name, ("kernel:0", "bias:0")) for name in AUX_LAYERS]
    return layers


def save_keras_weights(path, layers, keras_version=b"2.4.0", backend=b"tensorflow"):
    """keras hdf5_format.save_weights_to_hdf5_group: root attrs layer_names / backend / keras_version, one group per
    layer with attr weight_names and one float32 dataset per weight at <layer>/<weight name>."""
    root_attrs = _split_attr("layer_names", [n.encode("utf8") for n, _ in layers])
    root_attrs += [("backend", backend), ("keras_version", keras_version)]
    groups = [(lname, _split_attr("weight_names", [wn.encode("utf8") for wn, _ in ws]), ws) for lname, ws in layers]
    write_h5(path, root_attrs, groups)


def _load_attr_list(obj, name):
    """keras load_attributes_from_hdf5_group (handles the name0, name1, ... split)"""
    if name in obj.attrs:
        vals = list(np.atleast_1d(obj.attrs[name]))
    else:
        vals, i = [], 0
        while f"{name}{i}" in obj.attrs:
            vals += list(np.atleast_1d(obj.attrs[f"{name}{i}"]))
            i += 1
    return [v.decode("utf8") if isinstance(v, (bytes, np.bytes_)) else str(v) for v in vals]


def load_keras_weights(path):
    """-> [(layer name, [(weight name, float32 array)])] in the file's layer order, as keras
    hdf5_format.load_weights_from_hdf5_group walks it.  A full-model file (`model.save`) keeps the same tree under
    'model_weights'; that is followed too."""
    f = H5File(path)
    root = f["model_weights"] if ("layer_names" not in f.attrs and "layer_names0" not in f.attrs and "model_weights" in f) else f
    out = []
    for lname in _load_attr_list(root, "layer_names"):
        g = root[lname]
        ws = []
        for wn in (_load_attr_list(g, "weight_names") if g.attrs else []):
            d = g[wn]
            ws.append((wn, np.asarray(d.read(), dtype=np.float32)))
        out.append((lname, ws))
    return out


def flat_weights(layers):
    """the get_weights() list: layers with weights in file order, weights in weight_names order (keras matches by
    ORDER, not by name: hdf5_format.load_weights_from_hdf5_group)"""
    return [a for _, ws in layers for _, a in ws]
