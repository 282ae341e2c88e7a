"""Drop-in for the reference's modules/msg_func.py — tgnx.nn."""
from tgnx.nn import IdentityMessage  # noqa: F401
