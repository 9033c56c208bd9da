"""Training checkpoints with bit-exact resume (include/mobgs_hip.h K29, csrc/snapshot.hip).

`TrainableGaussians.save_ply` carries what eval.py reads -- the parameters and the decoder.  A run that is to be CONTINUED
also needs the Adam moments and step counts, the densification statistics, the deformation table, the learning rates as the
schedules left them, the blur kernel with its optimiser and rate, the caller's flags and the random generators:

    handle = save_training_state(path, stat=stat, dyn=dyn, blce=blce, iteration=it, counters={"flag_s": 0})
    ...                                   # training goes on: the file is written behind it
    handle.wait()
    st = load_training_state(path, device="cuda:0", training_args=opt)
    st.stat, st.dyn, st.blce, st.iteration, st.counters

A save is one mobgs_rows_snapshot launch per Gaussian set (every field of the table into ONE packed block, with the block's
integer checksum formed in the same pass) and one for the small tensors (module parameters, moments that live outside the
tables), all on the TRAINING stream -- ordered after the last optimiser step and before the next.  The blocks then travel to
pinned host memory on a side stream behind an event, and a host thread writes the file once they have arrived: the training
stream is held for the snapshot launches, not for the transfer or the write.  The file goes to a temporary name in the
target's directory and is renamed over it, so an interrupted save leaves the previous checkpoint whole.

What a checkpoint does NOT hold: binning hints, arena capacities, captured graphs (they do not change results and are
rebuilt; the caller records its GraphedCallable again), and the schedules' callables (rebuilt from `training_args`).

File: 32 bytes {magic, format version, header length, header byte sum}, a JSON header, then the blocks at 16-byte aligned
positions.  Everything the reader needs to refuse a damaged or foreign file is in the header: per block its length and the
64-bit sum of its 32-bit words (formed on the device when saving, by numpy when loading), per set the field list.
"""
from __future__ import annotations

import ctypes
import json
import math
import os
import random
import struct
import threading
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .densify import GROUPS, STATS

FORMAT_VERSION = 1
MAGIC = b"MOBGSCKP"
_PREAMBLE = struct.Struct("<8sIIQQ")   # magic, version, reserved, header bytes, sum of the header's bytes
SET_NAMES = ("stat", "dyn")
AUX = "aux"
# True: a save brackets its snapshot launches with timing events on the training stream and leaves them in
# handle.snapshot_events (scripts/checkpoint_timing.py: how long the stream is occupied)
TIME_SNAPSHOT = False


class CheckpointError(RuntimeError):
    """A checkpoint that cannot be used: the message names the check that failed and, where it applies, the set."""


# ---- packed layout: host arithmetic, the same as csrc/snapshot.hip's ------------------------------------------------------
def round16(nbytes: int) -> int:
    return (int(nbytes) + 15) & ~15


def pack_layout(row_bytes: List[int], n: int) -> Tuple[List[int], int]:
    """Slot offsets of the fields of one block and the block's length: field f occupies
    [offset_f, offset_f + round16(n * row_bytes_f)), slots follow each other in list order."""
    offsets, off = [], 0
    for rb in row_bytes:
        if rb < 0 or n < 0:
            raise ValueError(f"pack_layout: negative size (n = {n}, row_bytes = {rb})")
        offsets.append(off)
        off += round16(n * rb)
    return offsets, off


def word_sum(block) -> int:
    """Sum of the 32-bit words of a block (bytes-like or uint8 array whose length is a multiple of 4) modulo 2^64: what
    mobgs_rows_snapshot adds up on the device."""
    a = np.frombuffer(block, dtype=np.uint8) if not isinstance(block, np.ndarray) else block.reshape(-1).view(np.uint8)
    if a.size % 4:
        raise ValueError(f"word_sum: {a.size} bytes is not a whole number of 32-bit words")
    return int(a.view("<u4").sum(dtype=np.uint64))


def expected_fields() -> List[str]:
    """The fields every set of this build has, whatever its optimiser state: densify.GROUPS, the table, densify.STATS."""
    return [g for g, _ in GROUPS] + ["_deformation_table"] + list(STATS)


def check_fields(set_name: str, names: List[str]) -> None:
    """Refuse a field list that lacks a field of this build or holds one it does not know (a moment `<group>.exp_avg` /
    `.exp_avg_sq` of a known group is known)."""
    have = set(names)
    for f in expected_fields():
        if f not in have:
            raise CheckpointError(f"field list mismatch in set {set_name!r}: the checkpoint lacks the field {f!r} of this "
                                  "build (densify.GROUPS / STATS)")
    known = set(expected_fields()) | {f"{g}.{k}" for g, _ in GROUPS for k in ("exp_avg", "exp_avg_sq")}
    for f in names:
        if f not in known:
            raise CheckpointError(f"field list mismatch in set {set_name!r}: the checkpoint holds the field {f!r}, which "
                                  "this build does not have")


# ---- the file --------------------------------------------------------------------------------------------------------------
def _replace(tmp: str, path: str) -> None:
    os.replace(tmp, path)


def write_checkpoint(path: str, header: dict, blocks: List[Tuple[str, object]]) -> None:
    """Write header + blocks [(name, bytes-like)] to a temporary name next to `path`, then rename it over `path`.  A block's
    sum is taken from header["blocks"] when the caller has it (the device formed it), else computed here."""
    given = {b["name"]: b for b in header.get("blocks", [])}
    table, pos = [], 0
    for name, data in blocks:
        nbytes = memoryview(data).nbytes
        if nbytes % 16:
            raise ValueError(f"write_checkpoint: block {name!r} has {nbytes} bytes, not a multiple of 16")
        s = given[name]["sum"] if name in given and "sum" in given[name] else word_sum(data)
        table.append({"name": name, "offset": pos, "bytes": nbytes, "sum": int(s)})
        pos += nbytes
    header = dict(header, format=FORMAT_VERSION, blocks=table)
    text = json.dumps(header).encode("utf-8")
    text += b" " * (-(len(text) + _PREAMBLE.size) % 16)   # the blocks start at a multiple of 16
    directory = os.path.dirname(os.path.abspath(path))
    tmp = os.path.join(directory, f".{os.path.basename(path)}.tmp{os.getpid()}.{threading.get_ident()}")
    try:
        with open(tmp, "wb") as f:
            f.write(_PREAMBLE.pack(MAGIC, FORMAT_VERSION, 0, len(text), sum(text)))
            f.write(text)
            for _, data in blocks:
                f.write(data)
            f.flush()
            os.fsync(f.fileno())
        _replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def read_checkpoint(path: str) -> Tuple[dict, Dict[str, np.ndarray]]:
    """-> (header, {block name: uint8 array}); every check of the file itself: magic, format version, lengths (a truncated
    file), the header's sum and every block's checksum."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        pre = f.read(_PREAMBLE.size)
        if len(pre) < _PREAMBLE.size:
            raise CheckpointError(f"{path}: truncated: {size} bytes is shorter than the preamble")
        magic, version, _, hlen, hsum = _PREAMBLE.unpack(pre)
        if magic != MAGIC:
            raise CheckpointError(f"{path}: not a training checkpoint (magic {magic!r})")
        if version != FORMAT_VERSION:
            raise CheckpointError(f"{path}: format version {version}, this build reads version {FORMAT_VERSION}")
        if _PREAMBLE.size + hlen > size:
            raise CheckpointError(f"{path}: truncated: the header needs {hlen} bytes, the file has {size}")
        text = f.read(hlen)
        if sum(text) != hsum:
            raise CheckpointError(f"{path}: header checksum mismatch")
        header = json.loads(text.decode("utf-8"))
        start = _PREAMBLE.size + hlen
        blocks = {}
        for b in header["blocks"]:
            if start + b["offset"] + b["bytes"] > size:
                raise CheckpointError(f"{path}: truncated: the block of {b['name']!r} ends at byte "
                                      f"{start + b['offset'] + b['bytes']}, the file has {size}")
            f.seek(start + b["offset"])
            data = np.fromfile(f, dtype=np.uint8, count=b["bytes"])
            got = word_sum(data)
            if got != b["sum"]:
                raise CheckpointError(f"{path}: checksum mismatch in the block of {b['name']!r}: the file sums to "
                                      f"{got:#018x}, the header says {b['sum']:#018x}")
            blocks[b["name"]] = data
    return header, blocks


class SaveHandle:
    """What save_training_state returns: wait() joins the writer, result() re-raises what it raised (else -> the path)."""

    def __init__(self, path: str):
        self.path, self._error, self._thread, self._done = path, None, None, threading.Event()

    def _run(self, work):
        try:
            work()
        except BaseException as exc:  # noqa: BLE001  (handed to result())
            self._error = exc
        finally:
            self._done.set()

    def wait(self) -> "SaveHandle":
        if self._thread is not None:
            self._thread.join()
        self._done.wait()
        return self

    def done(self) -> bool:
        return self._done.is_set()

    def result(self) -> str:
        self.wait()
        if self._error is not None:
            raise self._error
        return self.path


def write_async(path: str, header: dict, blocks, ready=None, blocking: bool = False) -> SaveHandle:
    """write_checkpoint on a host thread (inline with blocking=True).  ready: called first, on that thread -- waits for the
    blocks to arrive and may return sums {block name: int} to put into the header.  blocks: a list, or a callable that
    yields it once `ready` has returned."""
    handle = SaveHandle(path)

    def work():
        sums = ready() if ready is not None else None
        hdr = dict(header)
        if sums:
            hdr["blocks"] = [{"name": k, "sum": v} for k, v in sums.items()]
        write_checkpoint(path, hdr, blocks() if callable(blocks) else blocks)

    if blocking:
        handle._run(work)
    else:
        handle._thread = threading.Thread(target=handle._run, args=(work,), name="mobgs-checkpoint", daemon=False)
        handle._thread.start()
    return handle


# ---- generators ----------------------------------------------------------------------------------------------------------
def capture_generators(device=None) -> dict:
    """The states of Python's `random`, torch's CPU generator and (device given) that device's generator, JSON-able."""
    version, words, gauss = random.getstate()
    out = {"python": [version, list(words), gauss], "torch_cpu": bytes(torch.get_rng_state().tolist()).hex()}
    if device is not None:
        out["torch_device"] = bytes(torch.cuda.get_rng_state(device).tolist()).hex()
    return out


def restore_generators(state: dict, device=None) -> None:
    version, words, gauss = state["python"]
    random.setstate((version, tuple(words), gauss))
    torch.set_rng_state(torch.tensor(list(bytes.fromhex(state["torch_cpu"])), dtype=torch.uint8))
    if device is not None and "torch_device" in state:
        torch.cuda.set_rng_state(torch.tensor(list(bytes.fromhex(state["torch_device"])), dtype=torch.uint8), device)


# ---- device side: descriptors and the two launches -----------------------------------------------------------------------
class _RowsField(ctypes.Structure):
    _fields_ = _lib._STRUCTS["MobgsRowsField"]  # read from include/mobgs_hip.h


def _upload(records) -> Tuple[torch.Tensor, torch.Tensor]:
    """A ctypes array -> (pinned host bytes, device bytes); the copy does not wait for the stream's earlier work."""
    host = torch.frombuffer(bytearray(bytes(records)), dtype=torch.uint8).pin_memory()
    return host, host.to("cuda", non_blocking=True)


def field_records(ptrs: List[int], row_bytes: List[int], offsets: List[int], zero_new: List[bool]):
    n = len(ptrs)
    arr = (_RowsField * max(n, 1))()
    for i in range(n):
        arr[i] = _RowsField(ptrs[i] if row_bytes[i] else 0, row_bytes[i], offsets[i], 1 if zero_new[i] else 0, 0)
    return arr


def rows_snapshot(records_dev: torch.Tensor, n_fields: int, n: int, longest: int, block: torch.Tensor,
                  sum_dev: torch.Tensor) -> None:
    """One mobgs_rows_snapshot launch on the current stream.  block: uint8 device tensor at a 16-byte aligned address that
    holds the layout's total; sum_dev: one int64 device element, zero on entry."""
    _lib.check(_lib.load().mobgs_rows_snapshot(n_fields, records_dev.data_ptr(), n, longest, block.data_ptr(),
                                               sum_dev.data_ptr(), _lib.stream()), "mobgs_rows_snapshot")


def rows_restore(records_dev: torch.Tensor, n_fields: int, n: int, capacity: int, longest: int,
                 block: torch.Tensor) -> None:
    _lib.check(_lib.load().mobgs_rows_restore(n_fields, records_dev.data_ptr(), n, capacity, longest, block.data_ptr(),
                                              _lib.stream()), "mobgs_rows_restore")


class _Plan:
    """Descriptors of one block for the tensors as they are now; rebuilt when a pointer, a size or n has changed."""

    def __init__(self):
        self.key, self.host, self.dev, self.offsets, self.total, self.longest, self.count = None, None, None, [], 0, 0, 0

    def update(self, ptrs, row_bytes, n, zero_new):
        key = (tuple(ptrs), tuple(row_bytes), n)
        if key != self.key:
            self.offsets, self.total = pack_layout(row_bytes, n)
            self.longest, self.count = max(row_bytes, default=0), len(ptrs)
            self.host, self.dev = _upload(field_records(ptrs, row_bytes, self.offsets, zero_new))
            self.key = key
        return self


# ---- a Gaussian set <-> header entry + block ---------------------------------------------------------------------------
def _dtype_name(dt: torch.dtype) -> str:
    return str(dt).replace("torch.", "")


def _table_entries(pc) -> List[dict]:
    """The table as table_state() would show it, WITHOUT adopting the optimiser's moments into fields (a save must not move
    what a DeviceAdam plan or a recorded graph points at): a moment the optimiser holds outside the fields is listed where it
    lies.  -> [{name, row_shape, dtype, row_bytes, zero_new, ptr}]"""
    n, out, seen = pc._n, [], {}
    if pc.optimizer is not None:
        for gr in pc.optimizer.param_groups:
            g = gr.get("name")
            if g in pc._fields and len(gr["params"]) == 1:
                st = pc.optimizer.state.get(gr["params"][0]) or {}
                for k in ("exp_avg", "exp_avg_sq"):
                    if k in st:
                        seen[f"{g}.{k}"] = st[k]

    def entry(name, t, zero_new):
        if not t.is_contiguous():
            raise RuntimeError(f"checkpoint: the field {name!r} is not contiguous")
        return {"name": name, "row_shape": list(t.shape[1:]), "dtype": _dtype_name(t.dtype),
                "row_bytes": math.prod(t.shape[1:]) * t.element_size(), "zero_new": bool(zero_new), "ptr": t.data_ptr()}

    for k, f in pc._fields.items():
        t = seen.pop(k, None)
        out.append(entry(k, t if t is not None else f.view(n), f.zero_new))
    for k, t in seen.items():
        out.append(entry(k, t, True))
    return out


def _set_meta(pc, entries: List[dict], plan: _Plan) -> dict:
    fields = [dict({k: v for k, v in e.items() if k != "ptr"}, offset=off) for e, off in zip(entries, plan.offsets)]
    return {"n": pc._n, "fields": fields, "capacity_factor": pc._factor, "spatial_lr_scale": pc.spatial_lr_scale,
            "percent_dense": pc.percent_dense, "is_dynamic": bool(pc.is_dynamic), "rows_coherent": int(pc.rows_coherent),
            "keep_sorted": bool(pc.keep_sorted), "has_pcd_order": getattr(pc, "pcd_order", None) is not None,
            "schedules": any(name in pc.__dict__ for name in pc._SCHEDULES), "total": plan.total}


def _plan_of_set(pc, plan: _Plan) -> Tuple[_Plan, List[dict]]:
    entries = _table_entries(pc)
    plan.update([e["ptr"] for e in entries], [e["row_bytes"] for e in entries], pc._n, [e["zero_new"] for e in entries])
    return plan, entries


def _optimizer_meta(opt, prefix: str, table_fields, tensors: dict) -> dict:
    """Groups with their current rate and hyper-parameters, per parameter its step count; moments that do not live in a set's
    table go into `tensors` (the small-tensor block)."""
    groups = []
    for gi, group in enumerate(opt.param_groups):
        entry = {k: (list(v) if isinstance(v, tuple) else v) for k, v in group.items() if k != "params"}
        in_table = (len(group["params"]) == 1 and f"{group.get('name')}.exp_avg" in table_fields)
        params = []
        for pj, p in enumerate(group["params"]):
            st = opt.state.get(p) or {}
            rec = {"step": float(st["step"]) if "step" in st else None, "moments": "exp_avg" in st,
                   "in_table": bool(in_table and "exp_avg" in st)}
            if rec["moments"] and not rec["in_table"]:
                for k in ("exp_avg", "exp_avg_sq"):
                    tensors[f"{prefix}/{gi}.{pj}/{k}"] = st[k]
            params.append(rec)
        groups.append({"group": entry, "params": params})
    return {"groups": groups}


def _restore_optimizer(opt, meta: dict, prefix: str, aux: dict, what: str, table=None) -> None:
    saved = meta["groups"]
    names = [g["group"].get("name") for g in saved]
    if any(n is not None for n in names):   # (a set's optimiser may hold fewer groups than training_setup() makes)
        opt.param_groups = [g for g in opt.param_groups if g.get("name") in names]
    if [g.get("name") for g in opt.param_groups] != names or \
            [len(g["params"]) for g in opt.param_groups] != [len(g["params"]) for g in saved]:
        raise CheckpointError(f"optimizer mismatch in {what}: the checkpoint's groups {names} are not the rebuilt "
                              f"optimiser's {[g.get('name') for g in opt.param_groups]}")
    for gi, (group, sv) in enumerate(zip(opt.param_groups, saved)):
        for k, v in sv["group"].items():
            group[k] = tuple(v) if isinstance(v, list) else v
        for pj, (p, rec) in enumerate(zip(group["params"], sv["params"])):
            opt.state.pop(p, None)
            if rec["step"] is None:
                continue
            st = {"step": torch.tensor(rec["step"], dtype=torch.float32)}
            if rec["in_table"]:
                for k in ("exp_avg", "exp_avg_sq"):
                    st[k] = table[f"{group['name']}.{k}"].view(table["#n"])
            elif rec["moments"]:
                for k in ("exp_avg", "exp_avg_sq"):
                    st[k] = aux[f"{prefix}/{gi}.{pj}/{k}"].reshape(p.shape).clone()
            opt.state[p] = st


_CTOR_KEY = {"xyz": ("p", "xyz"), "f_dc": ("p", "features_dc"), "f_t": ("p", "features_t"), "opacity": ("p", "opacity"),
             "scaling": ("p", "scaling"), "rotation": ("p", "rotation"), "f_rest": ("d", "f_rest"), "_deformation_table":
             ("d", "_deformation_table")}


def set_state_dict(pc) -> dict:
    """TrainableGaussians.state_dict(): {"meta", "block" (uint8 device tensor, the packed table), "sum", "optimizer",
    "tensors"} through ONE mobgs_rows_snapshot launch; "tensors" are clones of the moments that live outside the table (the
    decoder group's).  Reads the checksum back: synchronises."""
    plan, entries = _plan_of_set(pc, _Plan())
    dev = pc._fields["xyz"].buf[0].device
    with torch.cuda.device(dev):
        block = torch.empty(max(plan.total, 16), dtype=torch.uint8, device=dev)
        s = torch.zeros(1, dtype=torch.int64, device=dev)
        rows_snapshot(plan.dev, plan.count, pc._n, plan.longest, block, s)
    tensors: Dict[str, torch.Tensor] = {}
    opt = None if pc.optimizer is None else _optimizer_meta(pc.optimizer, "opt", {e["name"] for e in entries}, tensors)
    return {"meta": _set_meta(pc, entries, plan), "block": block[:plan.total], "sum": int(s.item()) & (2 ** 64 - 1),
            "optimizer": opt, "tensors": {k: t.detach().clone() for k, t in tensors.items()}}


def load_set_state(pc, state: dict) -> None:
    """TrainableGaussians.load_state_dict(): set_state_dict's result into this set -- the table through ONE
    mobgs_rows_restore launch, then (both sides have an optimiser) rates, hyper-parameters, step counts and moments, re-keyed
    through _publish(rekey=True)."""
    load_set_state_dict(pc, state)
    if pc.optimizer is not None and state.get("optimizer") is not None:
        _restore_optimizer(pc.optimizer, state["optimizer"], "opt", state.get("tensors", {}), "the set",
                           dict(pc._fields, **{"#n": pc._n}))
    pc._publish(rekey=pc.optimizer is not None)


def load_set_state_dict(pc, state: dict, set_name: str = "set") -> None:
    """TrainableGaussians.load_state_dict(): the table of `state` (set_state_dict's result, or a checkpoint's entry with its
    block on the device) into this set through ONE mobgs_rows_restore launch -- every field the set has; moments it has no
    field for yet get one when the set has an optimiser.  The optimiser is re-keyed through _publish(rekey=True)."""
    meta, block = state["meta"], state["block"]
    check_fields(set_name, [f["name"] for f in meta["fields"]])
    if "sum" in state and block.numel() and (int(_device_word_sum(block)) != state["sum"]):
        raise CheckpointError(f"checksum mismatch in the block of set {set_name!r}")
    n = int(meta["n"])
    dev = pc._fields["xyz"].buf[0].device
    from .densify import _Field
    if n > pc._capacity:
        pc._capacity = int(n * pc._factor) + 1024
        for f in pc._fields.values():
            f.grow(pc._capacity, 0)
    use = []
    for fm in meta["fields"]:
        f = pc._fields.get(fm["name"])
        shape, dtype = tuple(fm["row_shape"]), getattr(torch, fm["dtype"])
        if f is None:
            if pc.optimizer is None:
                continue   # (moments of a set that is loaded without an optimiser)
            f = pc._fields[fm["name"]] = _Field(torch.zeros((0,) + shape, dtype=dtype, device=dev), pc._capacity,
                                                bool(fm["zero_new"]))
        if f.row_shape != shape or f.dtype != dtype:
            raise CheckpointError(f"field list mismatch in set {set_name!r}: the field {fm['name']!r} is "
                                  f"{fm['dtype']} {shape} in the checkpoint and {_dtype_name(f.dtype)} {f.row_shape} here")
        use.append((f, fm))
    recs = field_records([f.buf[f.cur].data_ptr() for f, _ in use], [fm["row_bytes"] for _, fm in use],
                         [fm["offset"] for _, fm in use], [f.zero_new for f, _ in use])
    with torch.cuda.device(dev):
        _, rdev = _upload(recs)   # (the pinned source stays reserved until the copy has run: torch's host allocator)
        rows_restore(rdev, len(use), n, pc._capacity, max([fm["row_bytes"] for _, fm in use], default=0), block)
    pc._n = n
    from . import gaussian_renderer as _GR
    _GR.parameters_changed()


def _device_word_sum(block: torch.Tensor) -> int:
    return int(block.view(torch.int32).to(torch.int64).bitwise_and(0xFFFFFFFF).sum().item()) & (2 ** 64 - 1)


# ---- save ------------------------------------------------------------------------------------------------------------------
class _Stager:
    """Per device: the packed device blocks, their pinned host mirror, the checksums and the side stream.  ONE set of
    buffers: a second save waits for the first save's writer before it touches them."""

    def __init__(self, dev):
        self.dev = dev
        self.side = torch.cuda.Stream(dev)
        self.block = torch.empty(0, dtype=torch.uint8, device=dev)
        self.pinned = torch.empty(0, dtype=torch.uint8).pin_memory()
        self.sums = torch.zeros(3, dtype=torch.int64, device=dev)
        self.pinned_sums = torch.zeros(3, dtype=torch.int64).pin_memory()
        self.plans = {k: _Plan() for k in SET_NAMES + (AUX,)}
        self.pending: Optional[SaveHandle] = None

    def reserve(self, total: int):
        if self.block.numel() < total:
            size = int(total * 1.25) + 4096
            self.block = torch.empty(size, dtype=torch.uint8, device=self.dev)
            self.pinned = torch.empty(size, dtype=torch.uint8).pin_memory()


_stagers: Dict[str, _Stager] = {}


def _stager(dev) -> _Stager:
    key = str(dev)
    if key not in _stagers:
        _stagers[key] = _Stager(dev)
    return _stagers[key]


def release_staging() -> None:
    """Wait for the pending saves and drop the staging buffers (device and pinned blocks of the size of the last save)."""
    for st in _stagers.values():
        if st.pending is not None:
            st.pending.wait()
    _stagers.clear()


def _module_tensors(prefix: str, module, tensors: dict) -> List[str]:
    keys = []
    for k, t in module.state_dict().items():
        tensors[f"{prefix}/{k}"] = t
        keys.append(k)
    return keys


def save_training_state(path, *, stat, dyn, blce=None, device_adam=None, modules=None, iteration, counters=None,
                        blocking=False) -> SaveHandle:
    """Checkpoint of a training run after `iteration` completed iterations (module docstring).  stat / dyn:
    TrainableGaussians; blce: a blceKernel; device_adam: the DeviceAdam that steps their optimisers, if any
    (sync_to_host() is called first: one read-back of its counters); modules: {name: nn.Module} saved as state_dict();
    counters: the caller's JSON-able scalars.  Asynchronous unless blocking=True: the state is what the training stream holds
    when the snapshot launches run, i.e. after everything enqueued before this call and before anything enqueued after it."""
    path = os.fspath(path)
    if device_adam is not None:
        device_adam.sync_to_host()
    sets = {"stat": stat, "dyn": dyn}
    dev = stat._fields["xyz"].buf[0].device
    st = _stager(dev)
    if st.pending is not None:
        st.pending.wait()   # its staging buffers are free again (what it raised stays with its own handle)
        st.pending = None
    header = {"iteration": int(iteration), "counters": dict(counters or {}), "sets": {}, "optimizers": {},
              "device_adam": None if device_adam is None else {"iteration": int(device_adam.iteration),
                                                               "horizon": int(device_adam.horizon)}}
    tensors: Dict[str, torch.Tensor] = {}
    with torch.cuda.device(dev):
        for name, pc in sets.items():
            plan, entries = _plan_of_set(pc, st.plans[name])
            header["sets"][name] = _set_meta(pc, entries, plan)
            if pc.optimizer is not None:
                header["optimizers"][name] = _optimizer_meta(pc.optimizer, f"opt:{name}", {e["name"] for e in entries},
                                                             tensors)
            if getattr(pc, "pcd_order", None) is not None:
                tensors[f"pcd_order/{name}"] = pc.pcd_order
        header["decoder_shared"] = stat.rgbdecoder is dyn.rgbdecoder
        header["decoder"] = {"stat": _module_tensors("decoder/stat", stat.rgbdecoder, tensors)}
        if not header["decoder_shared"]:
            header["decoder"]["dyn"] = _module_tensors("decoder/dyn", dyn.rgbdecoder, tensors)
        if blce is not None:
            m = blce.model
            header["blce"] = {"num_views": int(m.num_views), "view_dim": int(m.view_embedder.shape[1]),
                              "num_warp": int(m.num_warp), "lr_factor": blce.lr_factor,
                              "keys": _module_tensors("blce", blce, tensors)}
            header["optimizers"]["blce"] = _optimizer_meta(blce.optimizer, "opt:blce", (), tensors)
        header["modules"] = {k: _module_tensors(f"module:{k}", mod, tensors) for k, mod in (modules or {}).items()}
        header["generators"] = capture_generators(dev)
        # the small tensors as the "rows" of a one-row table: one more launch of the same kernel
        small = {k: (t if t.is_cuda else t.to(dev)).detach() for k, t in tensors.items()}
        small = {k: (t if t.is_contiguous() else t.contiguous()) for k, t in small.items()}
        sizes = [t.numel() * t.element_size() for t in small.values()]
        aux = st.plans[AUX].update([t.data_ptr() for t in small.values()], sizes, 1, [False] * len(small))
        header[AUX] = [{"key": k, "dtype": _dtype_name(t.dtype), "shape": list(t.shape), "offset": off, "bytes": nb}
                       for (k, t), off, nb in zip(small.items(), aux.offsets, sizes)]
        plans = [st.plans["stat"], st.plans["dyn"], aux]
        rows = [stat._n, dyn._n, 1]
        bases, total = [], 0
        for p in plans:
            bases.append(total)
            total += p.total
        st.reserve(max(total, 16))
        train = torch.cuda.current_stream(dev)
        train.wait_stream(st.side)   # (the side stream's zeroing of the sums after the previous save)
        begin = None
        if TIME_SNAPSHOT:
            begin = torch.cuda.Event(enable_timing=True)
            begin.record(train)
        for i, (p, n) in enumerate(zip(plans, rows)):
            if p.count and p.total:
                rows_snapshot(p.dev, p.count, n, p.longest, st.block[bases[i]:], st.sums[i:])
        snap = torch.cuda.Event(enable_timing=begin is not None)
        snap.record(train)
        with torch.cuda.stream(st.side):
            st.side.wait_event(snap)
            st.pinned[:total].copy_(st.block[:total], non_blocking=True)
            st.pinned_sums.copy_(st.sums, non_blocking=True)
            arrived = torch.cuda.Event()
            arrived.record(st.side)
            st.sums.zero_()
    del small   # (what had to be copied to be contiguous has been read by launches enqueued on the training stream)

    def ready():
        arrived.synchronize()
        return {k: int(v) & (2 ** 64 - 1) for k, v in zip(SET_NAMES + (AUX,), st.pinned_sums.tolist())}

    def blocks():
        host = st.pinned.numpy()
        return [(k, host[b:b + p.total]) for k, b, p in zip(SET_NAMES + (AUX,), bases, plans)]

    handle = write_async(path, header, blocks, ready=ready, blocking=blocking)
    handle.snapshot_events = (begin, snap) if begin is not None else None
    st.pending = handle
    return handle


# ---- load ------------------------------------------------------------------------------------------------------------------
def _aux_tensors(header: dict, block: torch.Tensor) -> Dict[str, torch.Tensor]:
    out = {}
    for rec in header[AUX]:
        raw = block[rec["offset"]:rec["offset"] + rec["bytes"]]
        out[rec["key"]] = raw.view(getattr(torch, rec["dtype"])).reshape(rec["shape"])
    return out


def _new_set(meta: dict, decoder, device):
    """A TrainableGaussians with the checkpoint's shapes and zero rows' worth of content: the table is restored into it."""
    from .densify import TrainableGaussians
    n = int(meta["n"])
    by_name = {f["name"]: f for f in meta["fields"]}
    params, dynamic = {}, {}
    for g in expected_fields():
        if g in STATS:
            continue
        f = by_name[g]
        where, key = _CTOR_KEY.get(g, ("d", g))
        dtype = torch.bool if g == "_deformation_table" else getattr(torch, f["dtype"])
        (params if where == "p" else dynamic)[key] = torch.zeros((n,) + tuple(f["row_shape"]), dtype=dtype, device=device)
    pc = TrainableGaussians(params, dynamic, decoder=decoder, device=device, capacity_factor=meta["capacity_factor"])
    return pc


def _finish_set(pc, meta: dict, aux: dict, name: str):
    pc.is_dynamic = bool(meta["is_dynamic"])
    pc.percent_dense = meta["percent_dense"]
    pc.rows_coherent = int(meta["rows_coherent"])
    if meta["keep_sorted"]:
        pc.keep_sorted = True
    pc.pcd_order = aux[f"pcd_order/{name}"].clone() if meta["has_pcd_order"] else None


def load_training_state(path, *, device, training_args=None, decoder=None, stage="coarse", set_generators=True):
    """-> SimpleNamespace(stat, dyn, blce, modules, iteration, counters, device_adam, header): the objects of
    save_training_state rebuilt on `device` and the saved scalars.  Verifies the format version, every block's checksum and
    each set's field list against this build's densify.GROUPS / STATS; a mismatch raises CheckpointError naming the check and
    the set.  training_args: what training_setup() / setup_schedules() take (needed when the checkpoint holds optimisers:
    the schedules' callables are rebuilt from it; rates, hyper-parameters and step counts come from the file).  decoder: a
    fresh decoder module of the saved shape (default Sandwich(9, 3)).  modules: state dicts are returned as {name: {key:
    tensor}} for the caller's own load_state_dict().  A DeviceAdam is the caller's to build once its gradient storage
    exists: DeviceAdam(optimizers, schedules, horizon=..., first_iteration=state.iteration + 1) takes the step counts from
    the restored optimiser state, as rebuild() does.  The generators are set last.  Captured graphs are not part of a
    checkpoint: record the GraphedCallable again."""
    path = os.fspath(path)
    header, blocks = read_checkpoint(path)
    for name in SET_NAMES:
        if name not in header.get("sets", {}) or name not in blocks:
            raise CheckpointError(f"{path}: the checkpoint holds no set {name!r}")
        check_fields(name, [f["name"] for f in header["sets"][name]["fields"]])
    device = torch.device(device)
    from .helper_model import Sandwich
    with torch.cuda.device(device):
        dev_blocks = {k: torch.from_numpy(v).to(device) for k, v in blocks.items()}
        aux = _aux_tensors(header, dev_blocks[AUX]) if AUX in dev_blocks else {}
        dec = {"stat": decoder if decoder is not None else Sandwich(9, 3).to(device)}
        dec["dyn"] = dec["stat"] if header["decoder_shared"] else Sandwich(9, 3).to(device)
        for which, keys in header["decoder"].items():
            dec[which].load_state_dict({k: aux[f"decoder/{which}/{k}"] for k in keys})
        sets = {}
        for name in SET_NAMES:
            meta = header["sets"][name]
            pc = sets[name] = _new_set(meta, dec[name], device)
            pc.spatial_lr_scale = meta["spatial_lr_scale"]
            opt_meta = header["optimizers"].get(name)
            if opt_meta is not None:
                if training_args is None:
                    raise CheckpointError(f"{path}: set {name!r} was saved with its optimiser: load_training_state needs "
                                          "training_args to rebuild it")
                pc.training_setup(training_args)
                if meta["schedules"]:
                    pc.setup_schedules(training_args, stage)
            load_set_state_dict(pc, {"meta": meta, "block": dev_blocks[name]}, name)
            _finish_set(pc, meta, aux, name)
            if opt_meta is not None:
                table = dict(pc._fields, **{"#n": pc._n})
                _restore_optimizer(pc.optimizer, opt_meta, f"opt:{name}", aux, f"set {name!r}", table)
            pc._publish(rekey=True)
        blce = None
        if header.get("blce"):
            from .blce import blceKernel
            b = header["blce"]
            blce = blceKernel(num_views=b["num_views"], view_dim=b["view_dim"], num_warp=b["num_warp"]).to(device)
            blce.lr_factor = b["lr_factor"]
            blce.load_state_dict({k: aux[f"blce/{k}"] for k in b["keys"]})
            _restore_optimizer(blce.optimizer, header["optimizers"]["blce"], "opt:blce", aux, "the BLCE module")
        modules = {name: {k: aux[f"module:{name}/{k}"].clone() for k in keys}
                   for name, keys in header.get("modules", {}).items()}
        torch.cuda.current_stream(device).synchronize()   # (the restore launches read buffers this call owns)
    if set_generators:
        restore_generators(header["generators"], device)
    return SimpleNamespace(stat=sets["stat"], dyn=sets["dyn"], blce=blce, modules=modules,
                           iteration=int(header["iteration"]), counters=header["counters"],
                           device_adam=header.get("device_adam"), header=header)


def export_reference_layout(directory, *, stat, dyn, blce=None) -> List[str]:
    """The reference's Scene.save layout next to a checkpoint, through the existing save_ply: point_cloud.ply (the dynamic
    set) with the decoder as point_cloud.pt, point_cloud_static.ply, and blce.pth (the BLCE model's state_dict).  One save
    then serves a resume and eval.py.  -> the paths written."""
    directory = os.fspath(directory)
    os.makedirs(directory, exist_ok=True)
    out = [os.path.join(directory, "point_cloud.ply"), os.path.join(directory, "point_cloud_static.ply")]
    dyn.save_ply(out[0])
    stat.save_ply(out[1])
    out.append(out[0].replace(".ply", ".pt"))
    if blce is not None:
        out.append(os.path.join(directory, "blce.pth"))
        torch.save(blce.model.state_dict(), out[-1])
    return out
