"""Drop-in for the reference's modules/ package: the trainable per-operator modules of tgnx.nn (HIP forward and
backward), memory_module.TGNMemory / DyRepMemory over a device message store included."""
from tgnx.nn import *  # noqa: F401,F403
from tgnx.nn import __all__  # noqa: F401
