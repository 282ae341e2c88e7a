"""Drop-in for the reference's modules/emb_module.py — tgnx HIP path (forward and backward)."""
from tgnx.nn import GraphAttentionEmbedding, TimeEmbedding, TransformerConv  # noqa: F401
