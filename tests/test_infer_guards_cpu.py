"""The opening guards of the engine's inference passes (score, group_moments, gene_gram, rank_sums, latent_knn,
latent_kmeans, latent_silhouette, latent_louvain): the full text of every refusal, and which one wins when several
conditions hold at once.  Every pass checks in one order -- data-parallel world, (latent passes) no centre layer, ops without
the entry, no data -- so the error is that of the first condition in it that holds.  Nothing is computed: every call raises."""
import itertools

import numpy as np
import pytest

from helpers import make_problem
from _score_ref import ScoreRefOps
from _groups_ref import GroupRefOps
from _gram_ref import GramRefOps
from _ranksum_ref import RankSumRefOps
from _knn_ref import KnnRefOps
from _kmeans_ref import KmeansRefOps
from _silhouette_ref import SilhouetteRefOps
from _louvain_ref import LouvainRefOps
from dca_amd.engine import Engine
from oracle.cpu_ops import CpuRefOps

N, G, HS = 30, 9, (6, 3, 6)
CODES = (np.arange(N) % 3).astype(np.int32)
NO_CENTRE = (ValueError, 'No such layer: center (hidden_size=() has no latent representation)')

# pass -> (ops with the entry, the call, the conditions in the order the pass checks them: (condition, error, full text))
PASSES = {
    'score': (ScoreRefOps, lambda e: e.score(), (
        ('world', ValueError, 'dca_amd: score() does not apply to data-parallel runs (2 processes)'),
        ('ops', NotImplementedError, 'dca_amd: score() needs ops with nll_marginals (ops cpu-oracle has none)'),
        ('data', ValueError, 'dca_amd: score() needs the targets Y: this engine has none (load_data(X, None, sf) attaches '
                             'inputs only)'))),
    'group_moments': (GroupRefOps, lambda e: e.group_moments(CODES, 3), (
        ('world', ValueError, 'dca_amd: group_moments() does not apply to data-parallel runs (2 processes)'),
        ('ops', NotImplementedError, 'dca_amd: group_moments() needs ops with group_moments (ops cpu-oracle has none)'),
        ('data', ValueError, 'dca_amd: group_moments() needs data: load_data / attach_counts first'))),
    'gene_gram': (GramRefOps, lambda e: e.gene_gram(np.arange(4)), (
        ('world', ValueError, 'dca_amd: gene_gram() does not apply to data-parallel runs (2 processes)'),
        ('ops', NotImplementedError, 'dca_amd: gene_gram() needs ops with gram (ops cpu-oracle has none)'),
        ('data', ValueError, 'dca_amd: gene_gram() needs data: load_data / attach_counts first'))),
    'rank_sums': (RankSumRefOps, lambda e: e.rank_sums(CODES, 3), (
        ('world', ValueError, 'dca_amd: rank_sums() does not apply to data-parallel runs (2 processes)'),
        ('ops', NotImplementedError, 'dca_amd: rank_sums() needs ops with ranksum (ops cpu-oracle has none)'),
        ('data', ValueError, 'dca_amd: rank_sums() needs data: load_data / attach_counts first'))),
    'latent_knn': (KnnRefOps, lambda e: e.latent_knn(5), (
        ('world', ValueError, 'dca_amd: latent_knn() does not apply to data-parallel runs (2 processes)'),
        ('centre',) + NO_CENTRE,
        ('ops', NotImplementedError, 'dca_amd: latent_knn() needs ops with knn (ops cpu-oracle has none)'),
        ('data', ValueError, 'dca_amd: latent_knn() needs data: load_data / attach_counts first'))),
    'latent_kmeans': (KmeansRefOps, lambda e: e.latent_kmeans(3), (
        ('world', ValueError, 'dca_amd: latent_kmeans() does not apply to data-parallel runs (2 processes)'),
        ('centre',) + NO_CENTRE,
        ('ops', NotImplementedError, 'dca_amd: latent_kmeans() needs ops with kmeans_step (ops cpu-oracle has none)'),
        ('data', ValueError, 'dca_amd: latent_kmeans() needs data: load_data / attach_counts first'))),
    'latent_silhouette': (SilhouetteRefOps, lambda e: e.latent_silhouette(CODES, 3), (
        ('world', ValueError, 'dca_amd: latent_silhouette() does not apply to data-parallel runs (2 processes)'),
        ('centre',) + NO_CENTRE,
        ('ops', NotImplementedError, 'dca_amd: latent_silhouette() needs ops with silhouette (ops cpu-oracle has none)'),
        ('data', ValueError, 'dca_amd: latent_silhouette() needs data: load_data / attach_counts first'))),
    # latent_louvain checks the world and its own entry, then leaves the centre layer and the data to latent_knn: the
    # entry comes before the centre layer here, and the data refusal carries latent_knn's name
    'latent_louvain': (LouvainRefOps, lambda e: e.latent_louvain(5), (
        ('world', ValueError, 'dca_amd: latent_louvain() does not apply to data-parallel runs (2 processes)'),
        ('ops', NotImplementedError, 'dca_amd: latent_louvain() needs ops with louvain_level (ops cpu-oracle has none)'),
        ('centre',) + NO_CENTRE,
        ('data', ValueError, 'dca_amd: latent_knn() needs data: load_data / attach_counts first'))),
}


class TwoRanks:
    rank, world, dp = 0, 2, False


def _engine(ops_cls, held):
    """An engine on which exactly the conditions `held` hold."""
    hs = () if 'centre' in held else HS
    eng = Engine('zinb-conddisp', G, G, hs, True, 0.0, ops=(CpuRefOps if 'ops' in held else ops_cls)())
    if 'data' not in held:
        X, Y, sf, _ = make_problem(N, G, hs, 'zinb-conddisp', seed=4)
        eng.load_data(X, Y, sf)
    else:
        eng.n = N       # latent_louvain reads the cell count for its argument limits before latent_knn looks for data
    if 'world' in held:
        eng.comm = TwoRanks()
    return eng


def _cases():
    for name, (_, _, order) in PASSES.items():
        conds = [c[0] for c in order]
        for r in range(1, len(conds) + 1):
            for held in itertools.combinations(conds, r):
                yield pytest.param(name, held, id='%s-%s' % (name, '+'.join(held)))


@pytest.mark.parametrize('name,held', list(_cases()))
def test_the_first_condition_that_holds_is_the_error(name, held):
    ops_cls, call, order = PASSES[name]
    _, exc, text = next(c for c in order if c[0] in held)
    with pytest.raises(exc) as e:
        call(_engine(ops_cls, held))
    assert type(e.value) is exc and str(e.value) == text


def test_the_reference_ops_have_their_entry_and_the_plain_ones_none():
    for name, (ops_cls, _, order) in PASSES.items():
        entry = next(c[2] for c in order if c[0] == 'ops').split('needs ops with ')[1].split(' ')[0]
        assert hasattr(ops_cls, entry) and not hasattr(CpuRefOps, entry), (name, entry)
