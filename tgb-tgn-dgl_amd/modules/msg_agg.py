"""Drop-in for the reference's modules/msg_agg.py — tgnx HIP path (forward and backward)."""
from tgnx.nn import LastAggregator, MeanAggregator  # noqa: F401
