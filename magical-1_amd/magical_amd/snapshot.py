"""Env state snapshots: the blobs of mg_snapshot / mg_restore (include/magical_sim.h) as Python objects.

A `Snapshot` wraps one uint8 tensor: a 256-byte header and `len(snap)` env records (layout:
magical-1_amd/csrc/mg_snapshot.h).  The blob is opaque and relocatable: `.cpu()`, `.to(device)`, `.save(path)` /
`Snapshot.load(path)` (torch.save of the tensor alone -- nothing executable, loaded with weights_only=True) move
it between devices and processes; `VecMagicalEnv.restore` puts the recorded envs back.  The header fields are
parsed on the host (`snap.header`), so a blob of the wrong kind is refused before it reaches the GPU.

A `PoolSnapshot` is one blob per chunk of a `PipelinedVecEnv`, with the chunk bounds.
"""
import collections
import struct

import torch

from .native import NativeError

MAGIC = 0x4E53474D   # "MGSN"
VERSION = 1
HEADER_BYTES = 256
FRAME_BYTES = 96 * 96 * 3
# frames a record carries per GPU preprocessor id (mg_config.preproc): the rings of the stacked views, the current
# frame of a view without a ring, the allocentric static layer (mg_snapshot.h snap_frame_count)
FRAMES_PER_RECORD = {0: 0, 1: 6, 2: 8, 3: 6, 4: 5}

_FMT = "<II10i4q"
Header = collections.namedtuple(
    "Header", "magic version task rand_flags preproc max_bodies max_shapes max_cons max_arb max_ents nrows nframes "
              "state_bytes record_bytes count total_bytes")


def frame_bytes(preproc):
    """Bytes of LoRes frames in one record for GPU preprocessor id `preproc`."""
    return FRAMES_PER_RECORD[preproc] * FRAME_BYTES


def pack_header(**fields):
    """A 256-byte header (tests, tools): fields of `Header`; magic and version default to this library's."""
    fields.setdefault("magic", MAGIC)
    fields.setdefault("version", VERSION)
    return struct.pack(_FMT, *Header(**fields)).ljust(HEADER_BYTES, b"\0")


def parse_header(raw, nbytes=None):
    """Header of a blob from its first 256 bytes; raises NativeError for what is not a snapshot of this layout
    version, or (nbytes given) a blob shorter than its header says."""
    raw = bytes(raw)
    if len(raw) < HEADER_BYTES:
        raise NativeError(f"snapshot: a blob of {len(raw)} bytes is shorter than its {HEADER_BYTES}-byte header")
    h = Header(*struct.unpack_from(_FMT, raw))
    if h.magic != MAGIC:
        raise NativeError(f"snapshot: not a snapshot blob (magic {h.magic:#x}, expected {MAGIC:#x})")
    if h.version != VERSION:
        raise NativeError(f"snapshot: blob layout version {h.version}, this library reads {VERSION}")
    if h.count <= 0 or h.record_bytes <= 0 or h.total_bytes != HEADER_BYTES + h.count * h.record_bytes:
        raise NativeError("snapshot: inconsistent record count / record size / blob size in the header")
    if nbytes is not None and nbytes < h.total_bytes:
        raise NativeError(f"snapshot: truncated blob ({nbytes} bytes, the header says {h.total_bytes})")
    return h


class Snapshot:
    """`count` env records in one uint8 tensor (device or host)."""

    def __init__(self, blob, count=None):
        if not (isinstance(blob, torch.Tensor) and blob.dtype == torch.uint8 and blob.dim() == 1):
            raise TypeError("Snapshot: a 1-d uint8 tensor")
        self.blob = blob.contiguous()
        self._header = None
        self._count = count   # known to the env that took it: len() without reading the device

    @property
    def header(self):
        """The header fields (parsed and checked on the host; a device blob's 256 bytes are copied once)."""
        if self._header is None:
            self._header = parse_header(self.blob[:HEADER_BYTES].cpu().numpy().tobytes(), self.blob.numel())
        return self._header

    def __len__(self):
        return int(self._count if self._count is not None else self.header.count)

    @property
    def device(self):
        return self.blob.device

    def to(self, device):
        return Snapshot(self.blob.to(device), self._count)

    def cpu(self):
        return self.to("cpu")

    def save(self, path):
        torch.save(self.blob.cpu(), path)

    @classmethod
    def load(cls, path):
        snap = cls(torch.load(path, map_location="cpu", weights_only=True))
        snap.header   # refuse what is not a snapshot here, on the host
        return snap

    def tobytes(self):
        return self.blob.cpu().numpy().tobytes()

    @classmethod
    def frombytes(cls, data):
        snap = cls(torch.frombuffer(bytearray(data), dtype=torch.uint8))
        snap.header
        return snap


class PoolSnapshot:
    """A PipelinedVecEnv's state: one Snapshot per chunk; chunk k holds envs [bounds[k], bounds[k + 1]) in order."""

    def __init__(self, chunks, bounds):
        self.chunks, self.bounds = list(chunks), [int(b) for b in bounds]
        if len(self.chunks) + 1 != len(self.bounds):
            raise ValueError("PoolSnapshot: one blob per chunk")

    def __len__(self):
        return self.bounds[-1]

    def to(self, device):
        return PoolSnapshot([c.to(device) for c in self.chunks], self.bounds)

    def cpu(self):
        return self.to("cpu")

    def save(self, path):
        torch.save({"bounds": torch.tensor(self.bounds, dtype=torch.int64), "blobs": [c.blob.cpu() for c in self.chunks]},
                   path)

    @classmethod
    def load(cls, path):
        d = torch.load(path, map_location="cpu", weights_only=True)
        snap = cls([Snapshot(b) for b in d["blobs"]], d["bounds"].tolist())
        for c in snap.chunks:
            c.header
        return snap
