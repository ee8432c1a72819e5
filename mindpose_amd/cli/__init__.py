"""The recipe runner: ``config`` (command line + YAML recipe), ``train`` and ``eval`` (what the reference's tools/train.py and
tools/eval.py do, on this package's components)."""
