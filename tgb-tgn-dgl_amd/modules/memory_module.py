"""Drop-in for the reference's modules/memory_module.py — tgnx.nn (device message store, csrc/tgnx_memstore.hip)."""
from tgnx.nn import DyRepMemory, TGNMemory  # noqa: F401
