"""Drop-in for the reference's pyg_epoch_utils.py (train / test of the PyG TGN memory path) — fused HIP
step (tgnx/tgn_epoch.py; epoch_utils.train / test dispatch there for a TGN model as well)."""
from tgnx.tgn_epoch import compact, load_stream, observe, recommend, save_stream, test, train # noqa: F401
from tgnx.tgn_epoch import recommend_filtered  # noqa: F401
from tgnx.tgn_epoch import rank_stream  # noqa: F401
from tgnx.tgn_epoch import grow_nodes, observe_grow  # noqa: F401
from tgnx.tgn_epoch import embedding_table  # noqa: F401
from tgnx.tgn_epoch import similar  # noqa: F401
from tgnx.tgn_epoch import forget  # noqa: F401
from tgnx.tgn_epoch import explain, explain_recommendations  # noqa: F401
from tgnx.tgn_epoch import edgebank, tgb_negatives  # noqa: F401
from tgnx.nodeprop import test_node, train_node  # noqa: F401
from tgnx.nn import NodePredictor  # noqa: F401
from tgnx.tgn_epoch import edgebank_stream, edgebank_window, enable_pair_history, seen  # noqa: F401
