"""Drop-in for modules/time_enc.py (absent from the reference snapshot; PyG's TimeEncoder) — tgnx HIP path."""
from tgnx.nn import TimeEncoder  # noqa: F401
