"""The bodies of regda_amd.ops, one module per kernel family (csrc/*.hip); regda_amd/ops.py re-exports them."""
