"""Drop-in for the reference's modules/decoder.py — tgnx HIP path (forward and backward)."""
from tgnx.nn import LinkPredictor, NodePredictor  # noqa: F401
