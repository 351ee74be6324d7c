"""No device tests here.  The ``samples`` command, ``dtw_rank_batch`` and their GPU tests were
taken out after one of those tests hung inside the whole GPU suite with no cause found (DESIGN.md
section 24); what is left of that work is host code, tested in tests/test_samples.py."""
