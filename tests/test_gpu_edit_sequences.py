"""Edit sequences on the device: seeded random orders of append (both placement modes), removal, regraft, geometry edits by all four
calls (fyprt_update_mesh_vertices, fyprt_update_transforms with tuning key 22 = 0 and 1, fyprt_update_vertices), material and texture
edits, the cost readout, frames and denoiser probes on one live context, under the three builders of tuning key 12
(tests/edit_sequences.py).  After every edit: the edit's rule on the exports around it, the tree's invariants, lights and emissive list
against a fresh upload of the mirror's scene, 256 closest-hit and occlusion queries against a brute force over the scene's own
triangles; every frame against the oracle walking the current export with the frame state carried along, bit for bit; the denoisers
refused or not as the header says.  At the end of a sequence: device memory returns, and with key 12 = 0 the replay on a second context
is byte-equal and the last regraft equals its twin.
FYPRT_EDITSEQ_FIRST / FYPRT_EDITSEQ_LAST select another seed range (soak runs).
Measured on an MI355X: a cornell sequence of 20 ops takes 0.15 to 0.6 s, a hall_small sequence of 10 ops 0.9 to 1.5 s, the whole file
12 s."""
import pytest

import edit_sequences as es

pytestmark = pytest.mark.gpu

LEDGER = es.Ledger()
SCRIPTS = {"shrink and regrow": lambda: es.shrink_and_regrow(True), "grow past capacity": lambda: es.grow_past_capacity(True),
           "stale host vertices": es.stale_host_vertices, "links": lambda: es.links(True), "grafts spliced away": es.grafts_spliced_away,
           "removal after a lightless append": lambda: es.removal_after_a_lightless_append(True)}


@pytest.mark.parametrize("seed", es.seeds(6))
@pytest.mark.parametrize("key12", [0, 1, 2])
def test_random_edit_sequences_cornell(oracle_built, key12, seed):
    es.run_sequence(LEDGER, 0, "cornell", 1000 * key12 + seed, key12, geometry_ops=True, n_ops=20)


@pytest.mark.parametrize("seed", es.seeds(2))
@pytest.mark.parametrize("key12", [0, 2])
def test_random_edit_sequences_hall_small(oracle_built, key12, seed):
    """2108 nodes, 10 levels, the 1800-triangle drapes, levels of more than 256 nodes: the per-level launches of the partial refit."""
    es.run_sequence(LEDGER, 0, "hall_small", 1000 * key12 + 100 + seed, key12, geometry_ops=True, n_ops=10)


@pytest.mark.parametrize("key12", [0, 1, 2])
def test_random_edit_sequences_without_the_object_space_copy(oracle_built, key12):
    """Moves by fyprt_update_vertices only, removals always with their vertex ranges."""
    es.run_sequence(LEDGER, 0, "cornell", 1000 * key12 + 7, key12, geometry_ops=True, n_ops=20, object_copy=False)


@pytest.mark.parametrize("key12", [0, 2])
@pytest.mark.parametrize("script", list(SCRIPTS))
def test_scripted_edge_sequences(oracle_built, script, key12):
    es.run_sequence(LEDGER, 0, "cornell", 0, key12, ops=SCRIPTS[script]())


def test_edit_sequence_coverage():
    """(runs last in this file)  What the sequences above met: every op kind ten times, every order of a topology edit and the
    topology or geometry edit after it, the placement kinds, every branch of the prune rule, an emptied tree, a leaf-code root, grown
    node arrays, both refit paths."""
    missing = LEDGER.missing(device=True)
    assert not missing, missing
