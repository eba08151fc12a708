"""The catalogue of tests/helpers/rule_cases.py, checked without a GPU: every program compiles
within the device limits, RuleSet.evaluate and the host emulator of the device program agree on
it, it produces both routes, and the catalogue as a whole reaches every stack slot, MAX_OPS,
every opcode as a deciding operation and every feature index.  Then the proof that the catalogue
would notice a subtly wrong interpreter: each fault of rule_cases.MUTANTS, switched on in the
helper's own interpreter, changes the verdict of at least one program."""
import numpy as np
import pytest

from ccfd_demo_summit_amd.router.rules import MAX_OPS, MAX_STACK, run_device_program
from tests.helpers import rule_cases as rc

FEATURE_KINDS = ("mlp", "lr", "gbdt", "gbdt_d3", "forest")
PROBA_KINDS = ("gbdt", "gbdt_gl", "forest")


def _catalogues():
    """(label, view, rows as seen, CPU probabilities, name -> RuleSet) of every catalogue the GPU tests use."""
    out = []
    for kind in FEATURE_KINDS:
        for view in (rc.VIEWS if kind in ("mlp", "lr") else ("f32",)):
            out.append((f"{kind}/{view}", view, rc.rows()[view], rc.cpu_proba(kind, view),
                        rc.feature_catalogue(kind, view)))
    for kind in PROBA_KINDS:
        out.append((f"{kind}/proba", "f32", rc.rows()["f32"], rc.cpu_proba(kind), rc.proba_catalogue(kind)))
    return out


@pytest.fixture(scope="module")
def catalogues():
    return _catalogues()


def test_rows_have_the_tile_and_chunk_tails_and_the_edge_block():
    X = rc.rows()["f32"]
    assert len(X) == rc.N_ROWS == 17 * 16 + 1 == 4 * 64 + 17
    for v in rc.rows().values():
        for col, c in ((5, rc.C5), (6, rc.C6)):                  # several rows on the edge, most rows off it
            assert (v[:8, col] == np.float32(c)).all() and (v[8:, col] == np.float32(c)).sum() < 8
    chunks = -(-rc.N_V2 // 64)                                   # an odd number of two-chunk wave steps, 9 rows in the last
    assert rc.N_V2 == 262144 + 64 + 9 and (chunks // 2) % 2 == 1 and rc.N_V2 % 64 == 9


def test_every_program_compiles_agrees_with_the_emulator_and_gives_both_routes(catalogues):
    for label, view, X, p, cat in catalogues:
        for name, rs in cat.items():
            prog = rs.device_program()
            n_ops, depth, _, _ = rc.program_facts(prog)
            assert 0 < n_ops <= MAX_OPS and 0 < depth <= MAX_STACK, (label, name)
            want = rs.evaluate(p, X=X)
            np.testing.assert_array_equal(run_device_program(prog, p, X), want, err_msg=f"{label} {name}")
            np.testing.assert_array_equal(rc.Interp(view).run(prog, p, X), want, err_msg=f"{label} {name}")
            assert 0 < want.sum() < len(want), (label, name, int(want.sum()))


def test_one_program_per_feature_marks_about_half_the_rows(catalogues):
    for label, view, X, p, cat in catalogues:
        names = [k for k in cat if k.startswith("feature_")]
        assert len(names) == (1 if label.endswith("/proba") else 31), label
        for name in names:
            share = cat[name].evaluate(p, X=X).mean()
            assert 0.3 <= share <= 0.7, (label, name, share)


def test_packed_sweeps_are_full_length_default_fraud_and_cover_every_variable(catalogues):
    for label, view, X, p, cat in catalogues:
        if label.endswith("/proba"):
            head, _ = rc.program_ops(cat["sweep_p"].device_program())
            assert head.tolist() == [48, 1, 12, 2]
            continue
        seen = set()
        for name in rc.SWEEPS:
            head, ops = rc.program_ops(cat[name].device_program())
            assert head.tolist() == [48, 1, 12, 2], (label, name)
            seen |= {arg for op, arg, _ in ops if op == 1}
        assert seen == set(range(31)), label                     # proba and all 30 features


def test_catalogue_reaches_every_slot_every_opcode_and_every_feature(catalogues):
    for label, view, X, p, cat in catalogues:
        depths, feats, deciding, lengths = set(), set(), set(), set()
        for name, rs in cat.items():
            if name.startswith("random"):
                continue                                         # the hand-written programs alone suffice
            n_ops, depth, f, d = rc.program_facts(rs.device_program())
            depths.add(depth); feats |= f; deciding |= d; lengths.add(n_ops)
        assert {5, 6, 7, 8} <= depths, (label, depths)
        assert MAX_OPS in lengths, label
        assert set(rc.ALL_OPCODES) <= deciding, (label, sorted(set(rc.ALL_OPCODES) - deciding))
        if not label.endswith("/proba"):
            assert feats == set(range(30)), label
    # one program per depth: a fault in a single slot is localised
    cat = rc.feature_catalogue("mlp", "f32")
    assert [rc.program_facts(cat[f"slots{d}"].device_program())[1] for d in (5, 6, 7, 8)] == [5, 6, 7, 8]
    assert rc.program_facts(cat["slots8"].device_program())[0] == 18
    cat = rc.proba_catalogue("gbdt")
    assert [rc.program_facts(cat[f"slots{d}_p"].device_program())[1] for d in (5, 6, 7, 8)] == [5, 6, 7, 8]
    assert rc.program_facts(cat["slots8_p"].device_program())[0] == 18


def test_log1p_constant_is_far_from_every_row():
    for view in rc.VIEWS:
        a = rc.rows()[view][:, 29]
        c = rc._log1p_constant(a)
        v = np.log1p(a.astype(np.float64))
        assert (np.abs(v - np.float64(c)) > 16 * np.spacing(c)).all()
        assert 0.25 < (v > c).mean() < 0.75


def test_forty_random_rule_sets_without_log1p(catalogues):
    for label, view, X, p, cat in catalogues:
        if label.endswith("/proba"):
            continue
        names = [k for k in cat if k.startswith("random")]
        assert len(names) == rc.N_RANDOM == 40
        assert not any("log1p" in r.expr for k in names for r in cat[k].rules)


def _caught_by(mutant, catalogues, only=None):
    hits = []
    for label, view, X, p, cat in catalogues:
        if only is not None and not label.endswith(only):
            continue
        if rc.VIEW_MUTANTS.get(mutant, view) != view:
            continue
        it = rc.Interp(view, mutant)
        for name, rs in cat.items():
            if (it.run(rs.device_program(), p, X) != rs.evaluate(p, X=X)).any():
                hits.append(f"{label}:{name}")
    return hits


@pytest.mark.parametrize("mutant", rc.MUTANTS)
def test_catalogue_catches_mutant_interpreter(catalogues, mutant):
    hits = _caught_by(mutant, catalogues)
    print(f"{mutant}: caught by {len(hits)} programs, e.g. {hits[:6]}")
    assert hits, f"no catalogue program notices {mutant}"


# what binned rows can show: everything but the feature gathers
PROBA_MUTANTS = [m for m in rc.MUTANTS if not m.startswith(("feature_", "w64_", "f32_"))]


@pytest.mark.parametrize("mutant", PROBA_MUTANTS)
def test_proba_only_catalogue_catches_mutant_interpreter(catalogues, mutant):
    hits = _caught_by(mutant, catalogues, only="/proba")
    assert hits, f"no proba-only program notices {mutant}"


@pytest.mark.parametrize("k", [4, 5, 6, 7])
def test_slot_faults_are_localised(k):
    """The depth-d program is the shallowest that notices a fault in slot d - 1."""
    X, p = rc.rows()["f32"], rc.cpu_proba("mlp")
    cat = rc.feature_catalogue("mlp", "f32")
    for kind in ("pop", "push"):
        it = rc.Interp("f32", f"{kind}_slot{k}")
        for d in (5, 6, 7, 8):
            rs = cat[f"slots{d}"]
            differs = (it.run(rs.device_program(), p, X) != rs.evaluate(p, X=X)).any()
            assert differs == (d > k), (kind, k, d)
