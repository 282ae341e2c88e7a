"""Drop-in for the reference's modules/ package: the trainable per-operator modules of tgnx.nn (HIP forward and
backward).  memory_module.TGNMemory (a stateful memory with a device message store) is not provided: the fused
engine (tgnx.tgn) owns that path; compose MemoryCell + an aggregator + IdentityMessage instead."""
from tgnx.nn import *  # noqa: F401,F403
from tgnx.nn import __all__  # noqa: F401
