"""Edit sequences on host-only contexts (no GPU): seeded random orders of append (both placement modes), removal, regraft, material and
texture edits, the placement toggle and the cost readout, each step held against the edit's rule, the tree's invariants, a fresh upload
of the mirror's scene and 256 brute-force rays through the oracle's walk of the export; at the end of a sequence the replay on a second
context (byte-equal) and the twin of the last regraft (tests/edit_sequences.py).  Host-only contexts refuse the geometry calls, so
moves, frames and denoiser probes are the GPU file's.  24 x 24 ops on cornell, 3 x 12 on hall_small, the scripted edge sequences, and
the coverage ledger last."""
import pytest

import edit_sequences as es

LEDGER = es.Ledger()


@pytest.mark.parametrize("seed", es.seeds(24))
def test_random_edit_sequences_cornell(oracle_built, seed):
    es.run_sequence(LEDGER, -1, "cornell", seed, n_ops=24)


@pytest.mark.parametrize("seed", es.seeds(3))
def test_random_edit_sequences_hall_small(oracle_built, seed):
    es.run_sequence(LEDGER, -1, "hall_small", 100 + seed, n_ops=12)


SCRIPTS = {"shrink and regrow": lambda: es.shrink_and_regrow(False), "grow past capacity": lambda: es.grow_past_capacity(False),
           "links": lambda: es.links(False), "grafts spliced away": es.grafts_spliced_away,
           "removal after a lightless append": lambda: es.removal_after_a_lightless_append(False)}


@pytest.mark.parametrize("script", list(SCRIPTS))
def test_scripted_edge_sequences(oracle_built, script):
    es.run_sequence(LEDGER, -1, "cornell", 0, ops=SCRIPTS[script]())


def test_edit_sequence_coverage():
    """(runs last in this file)  What the sequences above met: every op kind ten times, every order of two topology edits, the
    placement kinds, every branch of the prune rule a host-built tree can show (all but "leaf partly emptied": the host builder makes one
    sub-tree per mesh), an emptied tree and a leaf-code root."""
    missing = LEDGER.missing(device=False)
    assert not missing, missing
