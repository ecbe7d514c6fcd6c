"""Plumbing every owner of a library handle shares: the symbols of one family (``at_<family>_*``, include/audiotoken_hip.h) looked up by name,
as ``_cabi.range_report`` does. PyTorch is used for device tensors and the caching allocator (workspace) only."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Optional, Union

import numpy as np
import torch

from . import _cabi


def _device_index(device: Union[str, torch.device]) -> int:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(
            f"audiotoken_amd runs on MI355X only (device 'cuda[:i]' under PyTorch-ROCm); got {device!r}. "
            "There is no CPU path in this package.")
    return dev.index if dev.index is not None else torch.cuda.current_device()


class LibHandle:
    """Mixin over ``lib``, ``handle`` and ``device`` of one family. A class that owns the handle gets them from ``_create`` and destroys the handle
    when it goes; one that borrows it (the EnCodec callables hold an ``_EncodecHandle``) provides ``lib`` and ``handle`` as properties."""

    FAMILY: str = ""                          # "encodec" | "w2vbert" | "hubert"
    ARITH: Optional[Dict[str, int]] = None    # names of the values of option "arith", where the family has it

    def _fn(self, name: str):
        return getattr(self.lib, f"at_{self.FAMILY}_{name}")

    def _create(self, device, packed, host_tensors: Callable[[], Dict[str, np.ndarray]], *finalize_args) -> None:
        """``create``, then either ``import_packed`` of ``packed = (meta, blob)`` or ``set_tensor`` of every host tensor + ``finalize``,
        then the class's ``_finish_init``."""
        self.lib = _cabi.load()
        self.device_index = _device_index(device)
        self.device = torch.device("cuda", self.device_index)
        tensors = host_tensors() if packed is None else None
        self.handle = self._fn("create")(self.device_index)
        if not self.handle:
            raise _cabi.HipLibraryError(f"at_{self.FAMILY}_create failed: {_cabi.last_error()}")
        if packed is not None:
            _cabi.import_packed(self.lib, self.FAMILY, self.handle, packed[0], packed[1].to(self.device))
        else:
            for name, arr in tensors.items():
                _cabi.set_tensor(self.lib, self._fn("set_tensor"), self.handle, name, arr)
            _cabi.check(self._fn("finalize")(self.handle, *finalize_args), f"at_{self.FAMILY}_finalize")
        self._finish_init()

    def __del__(self):
        h = self.__dict__.pop("handle", None)   # (a borrowed handle is a property, not an entry here)
        if h:
            self._fn("destroy")(h)

    def _init_call_state(self) -> None:
        self._ws: Optional[torch.Tensor] = None
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _workspace(self, nbytes: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None   # dropped before the larger one is allocated
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def last_status(self) -> int:
        """Status word of the LAST ``*_checked`` call: 0 = ok; bit 0 = a bounded wait inside the persistent LSTM kernel gave up (EnCodec); bit 1 = an
        activation exceeded the fp16 range of an f16x2 kernel; bit 2 = a NaN / infinity reached a quantiser (the encoders). Synchronises the device."""
        return int(self._status.item())

    def set_option(self, name: str, value) -> None:
        """Switches of the library (include/audiotoken_hip.h). The semantic families take "arith" as "f32" | "bf16x3" | "f16x2" (or 0/1/2)."""
        if isinstance(value, str):
            value = self.ARITH[value]
        _cabi.check(self._fn("set_option")(self.handle, name.encode(), int(value)), f"at_{self.FAMILY}_set_option({name})")

    def get_option(self, name: str) -> int:
        return int(self._fn("get_option")(self.handle, name.encode()))

    def range_report(self) -> Dict[str, float]:
        """{site: largest |x * scale| its split writers saw in the LAST call (semantic: over all layers)}: the measured headroom of the two-piece fp16
        arithmetic, which overflows at 65504 (0.0: the site did not run on that scheme). Synchronises the device."""
        return _cabi.range_report(self.lib, self.FAMILY, self.handle)

    # benchmark taps: HIP events recorded by the library on the launch stream, {group: (total ms, launches)}; off by default
    def enable_profile(self, on: bool) -> None:
        _cabi.check(self._fn("profile")(self.handle, 1 if on else 0), f"at_{self.FAMILY}_profile")

    def read_profile(self) -> Dict[str, tuple]:
        names = C.create_string_buffer(4096)
        ms = (C.c_float * 64)()
        ln = (C.c_int * 64)()
        n = self._fn("profile_read")(self.handle, names, 4096, ms, ln, 64)
        if n < 0:
            raise _cabi.HipLibraryError(f"at_{self.FAMILY}_profile_read failed: {_cabi.last_error()}")
        keys = names.value.decode().split("\n")[:n]
        return {k: (float(ms[i]), int(ln[i])) for i, k in enumerate(keys)}


class SemanticHandle(LibHandle):
    """What the two semantic encoders share beyond that: the per-layer range fallback's bookkeeping (audiotoken_amd/fallback.py)."""

    ARITH = {"f32": 0, "bf16x3": 1, "f16x2": 2}
    # a layer stays on bf16x3 from its PIN_AFTER-th overflowing batch on (fallback.semantic_ladder). AudioToken unpins at the end of
    # encode_batch_files and records what happened in `run_summary`.
    PIN_AFTER = 2
    LAYER_NOUN = "layer"   # "conformer" | "transformer", for messages

    def _finish_init(self) -> None:
        self.n_layers = self._fn("num_layers")(self.handle)
        if self.n_layers < self.output_layer:
            raise ValueError(f"checkpoint has {self.n_layers} {self.LAYER_NOUN} layers, output_layer={self.output_layer} needs that many")
        self._init_call_state()
        self.fallback_batches = 0    # batches `verified` repeated (fp16 range overflow)
        self.nonfinite_batches = 0   # batches whose activations held a NaN / infinity at the quantiser (status bit 2)
        self.pinned_layers = []      # layers `verified` moved to bf16x3 for good (their activations do not fit the fp16 range)
        self.layer_overflows = {}    # {layer: batches on which it overflowed}: a layer is pinned from the PIN_AFTER-th such batch on

    def export_packed(self):
        """(meta bytes, uint8 device blob): this finalized model for ``type(self)(packed=...)`` on the other ranks of a node."""
        return _cabi.export_packed(self.lib, self.FAMILY, self.handle, self.device)

    def layer_status(self):
        """Status flags of the LAST call per part (bit 1 = fp16 range overflow there), the OR over the part's split sites. semantic_m: one per conformer
        layer; semantic_s: [0] = conv feature encoder + positional conv, [1 + l] = transformer layer l. Synchronises."""
        buf = (C.c_int32 * 64)()
        n = self._fn("layer_status")(self.handle, buf, 64)
        if n < 0:
            raise _cabi.HipLibraryError(f"at_{self.FAMILY}_layer_status failed: {_cabi.last_error()}")
        return [int(buf[i]) for i in range(n)]

    def unpin_layers(self) -> None:
        """Return every layer the range fallback moved to bf16x3 to the handle's arithmetic."""
        for layer in set(self.pinned_layers):
            self.set_option(f"layer_arith:{layer}", -1)
        self.pinned_layers = []
        self.layer_overflows = {}
