"""mobgs_amd.checkpoint without a device: the file format (preamble, JSON header, checksummed blocks), what the reader refuses,
the atomic replace of the writer, the packed layout's arithmetic and the generators' round trip."""
import os
import random

import numpy as np
import pytest
import torch

from mobgs_amd import checkpoint as C


def _fields(names=None, moments=("xyz",)):
    names = list(names if names is not None else C.expected_fields())
    names += [f"{g}.{k}" for g in moments for k in ("exp_avg", "exp_avg_sq")]
    return [{"name": n, "row_shape": [3], "dtype": "float32", "row_bytes": 12, "zero_new": "." in n, "offset": 0}
            for n in names]


def _header(iteration=7):
    return {"iteration": iteration, "counters": {"flag_s": 1, "BEST_PSNR": 23.456789012345678, "lr": 1.6e-4 * 0.3},
            "sets": {"stat": {"n": 5, "fields": _fields()}, "dyn": {"n": 3, "fields": _fields()}}}


def _blocks(seed=0):
    rng = np.random.default_rng(seed)
    return [(name, rng.integers(0, 256, size, dtype=np.uint8)) for name, size in (("stat", 4096), ("dyn", 1600), ("aux", 16))]


def test_header_and_version_round_trip(tmp_path):
    path = str(tmp_path / "ckpt.mobgs")
    header, blocks = _header(), _blocks()
    C.write_checkpoint(path, header, blocks)
    got, data = C.read_checkpoint(path)
    assert got["format"] == C.FORMAT_VERSION and got["iteration"] == 7
    assert got["counters"] == header["counters"]             # floats survive JSON bit for bit
    assert got["sets"] == header["sets"]
    for (name, b), rec in zip(blocks, got["blocks"]):
        assert rec["name"] == name and rec["bytes"] == b.size and rec["sum"] == C.word_sum(b)
        assert np.array_equal(data[name], b)
    assert not [f for f in os.listdir(tmp_path) if f != "ckpt.mobgs"], "the temporary file was left behind"
    # another format version is refused by number
    raw = bytearray(open(path, "rb").read())
    raw[8:12] = (C.FORMAT_VERSION + 1).to_bytes(4, "little")
    open(path, "wb").write(raw)
    with pytest.raises(C.CheckpointError, match=f"format version {C.FORMAT_VERSION + 1}"):
        C.read_checkpoint(path)
    raw[0:8] = b"NOTACKPT"
    open(path, "wb").write(raw)
    with pytest.raises(C.CheckpointError, match="not a training checkpoint"):
        C.read_checkpoint(path)


def test_word_sum_is_the_uint64_sum_of_uint32_words():
    b = np.full(64, 0xFF, dtype=np.uint8)
    assert C.word_sum(b) == 16 * 0xFFFFFFFF                   # does not wrap at 32 bits
    assert C.word_sum(bytes(range(16))) == sum(int.from_bytes(bytes(range(16))[i:i + 4], "little") for i in range(0, 16, 4))
    with pytest.raises(ValueError):
        C.word_sum(b[:6])


@pytest.mark.parametrize("which", ["stat", "dyn"])
def test_flipped_byte_in_a_block_is_refused_by_the_checksum(tmp_path, which):
    path = str(tmp_path / "ckpt.mobgs")
    C.write_checkpoint(path, _header(), _blocks())
    header, _ = C.read_checkpoint(path)
    rec = next(b for b in header["blocks"] if b["name"] == which)
    size = os.path.getsize(path)
    start = size - sum(b["bytes"] for b in header["blocks"])
    raw = bytearray(open(path, "rb").read())
    raw[start + rec["offset"] + rec["bytes"] // 2] ^= 0x10
    open(path, "wb").write(raw)
    with pytest.raises(C.CheckpointError, match=f"checksum mismatch in the block of '{which}'"):
        C.read_checkpoint(path)


def test_flipped_byte_in_the_header_is_refused(tmp_path):
    path = str(tmp_path / "ckpt.mobgs")
    C.write_checkpoint(path, _header(), _blocks())
    raw = bytearray(open(path, "rb").read())
    raw[40] ^= 0x01
    open(path, "wb").write(raw)
    with pytest.raises(C.CheckpointError, match="header checksum"):
        C.read_checkpoint(path)


@pytest.mark.parametrize("keep", [0, 20, 200, -1, -1700])
def test_truncated_file_is_refused(tmp_path, keep):
    path = str(tmp_path / "ckpt.mobgs")
    C.write_checkpoint(path, _header(), _blocks())
    raw = open(path, "rb").read()
    open(path, "wb").write(raw[:keep] if keep else b"")
    with pytest.raises(C.CheckpointError, match="truncated"):
        C.read_checkpoint(path)


def test_load_refuses_a_checkpoint_that_lacks_a_field(tmp_path):
    """The whole reader: a well-formed file whose dynamic set was written by a build without `motion` is refused before
    anything touches a device, and the error names the check, the set and the field."""
    path = str(tmp_path / "ckpt.mobgs")
    header = _header()
    header["sets"]["dyn"]["fields"] = _fields([n for n in C.expected_fields() if n != "motion"])
    C.write_checkpoint(path, header, _blocks())
    with pytest.raises(C.CheckpointError, match=r"field list mismatch in set 'dyn'.*lacks the field 'motion'"):
        C.load_training_state(path, device="cuda:0")


@pytest.mark.parametrize("missing", ["motion", "_deformation_table", "max_radii2D"])
def test_missing_field_is_refused_by_name(missing):
    names = [n for n in C.expected_fields() if n != missing]
    with pytest.raises(C.CheckpointError, match=rf"set 'dyn'.*lacks the field '{missing}'"):
        C.check_fields("dyn", [f["name"] for f in _fields(names)])
    C.check_fields("dyn", [f["name"] for f in _fields()])     # the full list, with moments, passes
    with pytest.raises(C.CheckpointError, match="holds the field 'sh_extra'"):
        C.check_fields("stat", C.expected_fields() + ["sh_extra"])


def test_failed_write_leaves_the_previous_checkpoint(tmp_path, monkeypatch):
    path = str(tmp_path / "ckpt.mobgs")
    first = C.write_async(path, _header(iteration=5), _blocks(1))
    assert first.result() == path

    class Interrupted(Exception):
        pass

    def fail(tmp, dst):
        assert os.path.exists(tmp) and os.path.dirname(tmp) == os.path.dirname(dst)   # same directory: rename is atomic
        raise Interrupted("simulated: the writer died before the rename")

    monkeypatch.setattr(C, "_replace", fail)
    second = C.write_async(path, _header(iteration=9), _blocks(2))
    second.wait()
    assert second.done()
    with pytest.raises(Interrupted):
        second.result()
    monkeypatch.undo()
    header, data = C.read_checkpoint(path)
    assert header["iteration"] == 5 and np.array_equal(data["stat"], _blocks(1)[0][1])
    assert os.listdir(tmp_path) == ["ckpt.mobgs"], "the failed save's temporary file was left behind"
    # blocking=True: the same through the same handle, inline
    monkeypatch.setattr(C, "_replace", fail)
    with pytest.raises(Interrupted):
        C.write_async(path, _header(iteration=9), _blocks(2), blocking=True).result()


def test_pack_layout():
    offsets, total = C.pack_layout([12, 1, 0, 144, 2], 65)
    # 65 rows: 780 -> 784, 65 -> 80, 0, 9360, 130 -> 144
    assert offsets == [0, 784, 864, 864, 10224] and total == 10224 + 144
    assert all(o % 16 == 0 for o in offsets) and total % 16 == 0
    assert C.pack_layout([12, 4], 0) == ([0, 0], 0)
    assert C.pack_layout([], 5) == ([], 0)
    with pytest.raises(ValueError):
        C.pack_layout([4, -1], 3)


def test_generator_states_round_trip():
    random.seed(123)
    torch.manual_seed(456)
    random.random(), torch.rand(3), random.gauss(0, 1)       # (mid-stream, with a cached gaussian)
    state = C.capture_generators()
    import json
    state = json.loads(json.dumps(state))                     # as the header stores it
    want = (random.random(), random.gauss(0, 1), random.randint(0, 10 ** 9), torch.rand(5), torch.randn(4),
            torch.randperm(9))
    random.seed(1), torch.manual_seed(1)
    C.restore_generators(state)
    got = (random.random(), random.gauss(0, 1), random.randint(0, 10 ** 9), torch.rand(5), torch.randn(4),
           torch.randperm(9))
    for a, b in zip(want, got):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
