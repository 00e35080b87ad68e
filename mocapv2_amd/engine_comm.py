"""The exchange step of MocapContext (abi_comm.hip): one all-gather of centroid records, RCCL over xGMI."""
import ctypes as C

import torch

from . import _abi
from ._dev import _ptr, _stream


def comm_available():
    """Local check, no communication: can this process load RCCL (mocap_comm_available)?  Raises MocapError when not."""
    _abi.check(_abi.load().mocap_comm_available())
    return True


def comm_unique_id():
    """MOCAP_COMM_ID_BYTES opaque bytes (ncclGetUniqueId) for MocapContext.comm_init; call on rank 0 only."""
    buf = (C.c_char * _abi.COMM_ID_BYTES)()
    _abi.check(_abi.load().mocap_comm_unique_id(C.cast(buf, C.c_void_p)))
    return bytes(buf)


class CommStage:
    def comm_init(self, unique_id, rank, world):
        """Collective over all ranks: create this context's RCCL communicator from the bytes rank 0 got from
        `comm_unique_id()` (handed around by the host, e.g. through torch.distributed)."""
        buf = (C.c_char * _abi.COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        _abi.check(self.lib.mocap_comm_init(self._h, C.cast(buf, C.c_void_p), int(rank), int(world)))
        self.comm_world = int(world)

    def comm_share(self, src):
        """Local: use the communicator of `src` (another context of this rank on the same GPU) -- one communicator per rank,
        whatever the number of batches in flight; the library orders the all-gathers issued through it."""
        _abi.check(self.lib.mocap_comm_share(self._h, src._h))
        self.comm_world = src.comm_world

    def comm_destroy(self):
        _abi.check(self.lib.mocap_comm_destroy(self._h))
        self.comm_world = 1

    def allgather_centroids(self, local, out=None):
        """local: this rank's centroid records (int32, contiguous, on this GPU) -> [world * len(local), ...] on every
        rank, in rank order; asynchronous on the current stream."""
        assert local.is_cuda and local.is_contiguous() and local.dtype == torch.int32
        if out is None:
            out = torch.empty((self.comm_world * local.shape[0],) + tuple(local.shape[1:]), dtype=torch.int32, device=local.device)
        assert out.is_contiguous() and out.numel() == self.comm_world * local.numel() and out.dtype == torch.int32
        _abi.check(self.lib.mocap_allgather_centroids(self._h, _ptr(local), _ptr(out), local.numel(), _stream()))
        return out
