"""Command line of the reference (``dca input outputdir [flags]``, dca/__main__.py:18-154) on the
MI355X path: same positionals, flag names, defaults and output files.  The option table below
restates the reference's flag set; ``--mcv`` (beyond the reference) runs dca_amd/mcv.py; ``--neighbors K`` (beyond the reference) writes the latent space's
k-nearest-neighbour lists (dca_amd/neighbors.py); ``--groupstats FILE`` (beyond the reference) compares groups of cells on the
denoised expression (dca_amd/groups.py; ``--groupstats-method wilcoxon``: by the rank-sum test); ``--kmeans K`` (beyond the reference) clusters the latent space (dca_amd/cluster.py);
``--silhouette {kmeans,groups}`` (beyond the reference) scores such a clustering (dca_amd/silhouette.py);
``--genecorr FILE`` (beyond the reference) correlates genes on the denoised expression (dca_amd/genecorr.py);
``--hyper*`` runs dca_amd/hyper.py (the search space and outputs of
dca/hyper.py with hyperopt's TPE restated in dca_amd/tpe.py); ``--tensorboard`` is accepted for
command-line compatibility and ignored.
"""
import argparse
import sys

# (flags, kwargs) -- names / defaults as dca/__main__.py:31-136
_OPTIONS = [
    (('--normtype',), dict(type=str, default='zheng', help='size factor estimation: deseq | zheng (parsed, unused -- as in the reference)')),
    (('-t', '--transpose'), dict(dest='transpose', action='store_true', help='input is cell x gene (default: gene x cell)')),
    (('--testsplit',), dict(dest='testsplit', action='store_true', help='hold one fold out as a test set')),
    (('--type',), dict(type=str, default='nb-conddisp', help='autoencoder type (see dca_amd.network.AE_types)')),
    (('--threads',), dict(type=int, default=None, help='host threads of the native host stages (the reference sized TensorFlow CPU pools with it; the step runs on the GPU)')),
    (('-b', '--batchsize'), dict(type=int, default=32, help='batch size (default: 32)')),
    (('--sizefactors',), dict(dest='sizefactors', action='store_true', help='normalise means by library size (default)')),
    (('--nosizefactors',), dict(dest='sizefactors', action='store_false')),
    (('--norminput',), dict(dest='norminput', action='store_true', help='zero-mean normalise the input (default)')),
    (('--nonorminput',), dict(dest='norminput', action='store_false')),
    (('--loginput',), dict(dest='loginput', action='store_true', help='log-transform the input (default)')),
    (('--nologinput',), dict(dest='loginput', action='store_false')),
    (('-d', '--dropoutrate'), dict(type=str, default='0.0', help='dropout rate(s), comma separated')),
    (('--batchnorm',), dict(dest='batchnorm', action='store_true', help='batch normalisation (default)')),
    (('--nobatchnorm',), dict(dest='batchnorm', action='store_false')),
    (('--l2',), dict(type=float, default=0.0)),
    (('--l1',), dict(type=float, default=0.0)),
    (('--l2enc',), dict(type=float, default=0.0)),
    (('--l1enc',), dict(type=float, default=0.0)),
    (('--ridge',), dict(type=float, default=0.0, help='L2 penalty on the dropout probabilities')),
    (('--gradclip',), dict(type=float, default=5.0, help='clip gradient values (default: 5.0)')),
    (('--activation',), dict(type=str, default='relu')),
    (('--optimizer',), dict(type=str, default='RMSprop')),
    (('--init',), dict(type=str, default='glorot_uniform')),
    (('-e', '--epochs'), dict(type=int, default=300)),
    (('--earlystop',), dict(type=int, default=15)),
    (('--reducelr',), dict(type=int, default=10)),
    (('-s', '--hiddensize'), dict(type=str, default='64,32,64')),
    (('--inputdropout',), dict(type=float, default=0.0)),
    (('-r', '--learningrate'), dict(type=float, default=None)),
    (('--saveweights',), dict(dest='saveweights', action='store_true')),
    (('--no-saveweights',), dict(dest='saveweights', action='store_false')),
    (('--hyper',), dict(dest='hyper', action='store_true')),
    (('--hypern',), dict(dest='hypern', type=int, default=1000)),
    (('--hyperepoch',), dict(dest='hyperepoch', type=int, default=100)),
    (('--hypermcv',), dict(dest='hypermcv', type=float, default=None, metavar='FRACTION',
                           help='with --hyper: rank the trials by molecular cross-validation -- fit on a binomial FRACTION of '
                                'every count, minimise the likelihood of the held-out molecules -- instead of val_loss')),
    (('--debug',), dict(dest='debug', action='store_true')),
    (('--tensorboard',), dict(dest='tensorboard', action='store_true')),
    (('--checkcounts',), dict(dest='checkcounts', action='store_true')),
    (('--nocheckcounts',), dict(dest='checkcounts', action='store_false')),
    (('--denoisesubset',), dict(dest='denoisesubset', type=str, help='file with gene names (one per line) to denoise')),
    (('--score',), dict(dest='score', action='store_true',
                        help='after the result files: the fitted model\'s mean negative log-likelihood per cell (cell_nll.tsv, train and '
                             'test cells alike) and per gene (gene_nll.tsv), computed on the GPU')),
    (('--neighbors',), dict(dest='neighbors', type=int, default=None, metavar='K',
                            help='after the result files: every cell\'s K nearest other cells in the latent space, exact and '
                                 'Euclidean, computed on the GPU (knn_indices.tsv: 0-based cell numbers, knn_distances.tsv)')),
    (('--groupstats',), dict(dest='groupstats', type=str, default=None, metavar='FILE',
                             help='after the result files: groups of cells compared on the denoised expression, the pass over '
                                  'the cells computed on the GPU.  FILE: tab-separated, no header, cell name and label per line '
                                  '(cells not listed are left out).  Writes group_sizes.tsv, group_mean.tsv, group_var.tsv, '
                                  'group_scores.tsv (Welch t against the rest), group_pvals_adj.tsv, group_logfoldchanges.tsv '
                                  'of the log1p of the mean without size factors')),
    (('--groupstats-method',), dict(dest='groupstats_method', choices=('t-test', 'wilcoxon'), default=None,
                                    help='the test of --groupstats FILE / --kmeansstats: t-test (default: Welch t) or wilcoxon '
                                         '(the rank-sum test, every gene sorted on the GPU; group_scores.tsv holds its z score '
                                         'and group_auroc.tsv is written as well)')),
    (('--groupstats-tie-correct',), dict(dest='groupstats_tie_correct', action='store_true',
                                         help='with --groupstats-method wilcoxon: the tie correction of the variance')),
    (('--kmeans',), dict(dest='kmeans', type=int, default=None, metavar='K',
                         help='after the result files: k-means of the cells in the latent space into K clusters (1 .. 256), '
                              'computed on the GPU (kmeans_labels.tsv: cell name and label per line, the format --groupstats '
                              'reads; kmeans_centers.tsv)')),
    (('--kmeansstats',), dict(dest='kmeansstats', action='store_true',
                              help='with --kmeans: the group_*.tsv files of --groupstats for the k-means clusters (not together '
                                   'with --groupstats)')),
    (('--kmeans-seed',), dict(dest='kmeans_seed', type=int, default=0, metavar='N', help='seed of the k-means++ draws (default: 0)')),
    (('--louvain',), dict(dest='louvain', action='store_true',
                          help='after the result files: Louvain communities of the cells\' neighbour graph in the latent space '
                               '(--neighbors K other cells each, 15 when absent), computed on the GPU; the number of clusters '
                               'follows from the graph (louvain_labels.tsv: cell name and label per line, the format '
                               '--groupstats reads) and the modularity is printed')),
    (('--louvain-resolution',), dict(dest='louvain_resolution', type=float, default=None, metavar='R',
                                     help='with --louvain: the resolution of the modularity, 1/1024 .. 64 (default: 1.0; '
                                          'larger: more, smaller clusters)')),
    (('--louvainstats',), dict(dest='louvainstats', action='store_true',
                               help='with --louvain: the group_*.tsv files of --groupstats for the Louvain clusters (not '
                                    'together with --groupstats or --kmeansstats)')),
    (('--silhouette',), dict(dest='silhouette', choices=('kmeans', 'groups', 'louvain'), default=None,
                             help='after the result files: the silhouette coefficient of every cell in the latent space, '
                                  'computed on the GPU, under the clusters of --kmeans K (kmeans) or the labels of --groupstats '
                                  'FILE (groups); writes silhouette.tsv (cell, label, silhouette, nearest other cluster) and '
                                  'silhouette_clusters.tsv (label, size, mean silhouette) and prints the overall mean')),
    (('--genecorr',), dict(dest='genecorr', type=str, default=None, metavar='FILE',
                           help='after the result files: Pearson correlation between the genes FILE names (one per line, at '
                                'most 8192, read as --denoisesubset reads its file) on the denoised mean over all cells, the '
                                'pass over the cells computed on the GPU; writes gene_corr.tsv (genes x genes, in the order of '
                                'the input)')),
    (('--genecorr-log1p',), dict(dest='genecorr_log1p', action='store_true',
                                 help='with --genecorr: correlate log1p of the mean without size factors')),
    (('--mcv',), dict(dest='mcv', type=float, default=None, metavar='FRACTION',
                      help='molecular cross-validation instead of the denoising run: thin every count binomially, fit on FRACTION '
                           'of the molecules with the network and training flags given, score the held-out rest of every cell; '
                           'writes mcv.json, gene_mcv_nll.tsv and cell_mcv_nll.tsv')),
]

_DEFAULTS = dict(transpose=False, testsplit=False, saveweights=False, sizefactors=True, batchnorm=True,
                 checkcounts=True, norminput=True, hyper=False, debug=False, tensorboard=False,
                 loginput=True, score=False, kmeansstats=False, louvain=False, louvainstats=False, silhouette=None, genecorr_log1p=False,
                 groupstats_tie_correct=False)


def build_parser():
    parser = argparse.ArgumentParser(prog='dca', description='Autoencoder')
    parser.add_argument('input', type=str, help='raw counts: TSV/CSV (gene x cell unless -t), Matrix Market (.mtx, .mtx.gz) or H5AD')
    parser.add_argument('outputdir', type=str, help='output directory')
    for flags, kw in _OPTIONS:
        parser.add_argument(*flags, **kw)
    parser.set_defaults(**_DEFAULTS)
    return parser


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    from .train import train_with_args
    train_with_args(args)


if __name__ == '__main__':
    main(sys.argv[1:])
