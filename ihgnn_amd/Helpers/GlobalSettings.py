"""Process-wide settings: the knobs the reference keeps as class attributes of ``Gs`` / string tags of ``Gsv``
(reference ``Helpers/GlobalSettings.py:6-109``).  Only the attributes the hypergraph path and its driver read
are carried; values are the reference defaults.
"""
import torch.nn as nn


class Gsv:
    mean, activation, rnn = 'mean', 'activation', 'rnn'
    gru = 'gru'      # the recurrent query model that runs here (nn.GRU over the words in order); rnn stays the reference's refused placeholder
    concat, product = 'concatenation', 'product'
    graph_uqi, graph_only_uq, graph_only_ui, graph_only_qi = 'uqi', 'uq', 'ui', 'qi'


class Gs:
    use_valid_dataset = True
    adjust_learning_rate = True          # lr *= 0.98 per epoch once avg loss < 0.008 while lr > 4e-4
    lambda_muq_for_hem = 0.5

    batch_size = 100                     # positives per batch; rows per batch = batch_size * (1 + negatives)
    batch_size_times = 1
    learning_rate = 0.001
    embedding_size = 32
    weight_decay = 0

    graph_completeness = Gsv.graph_uqi
    long_tail_stat_fn = None

    random_negative_sample_size = 10
    non_random_negative_sample_size = 0
    negative_sample_size = random_negative_sample_size + non_random_negative_sample_size

    class Gnn:
        # GATLayer (GnnLayers.py:65-86): the reference assigns each twice or three times and the last assignment wins (GlobalSettings.py:59-66)
        gat_head = Gsv.concat            # or Gsv.product
        gat_activation = (nn.LeakyReLU, 'leaky_relu')      # or (nn.ReLU, 'relu'), (nn.Tanh, 'tanh')

    class Query:
        transform = Gsv.mean             # or Gsv.activation: nn.Linear(d, d) + transform_activation on the bag mean (EmbeddingLayers.py:37-44); Gsv.gru: nn.GRU(d, d) over the words in file order, its last state; Gsv.rnn raises, as in the reference
        transform_activation = nn.ReLU   # or nn.Tanh (the reference's other assignment, GlobalSettings.py:74-76)

    class Prediction:
        use_cosine_similarity = False

    class Training:
        loss = 'bce'                     # not in the reference (whose only objective is nn.BCEWithLogitsLoss over a positive and its negatives): 'bpr' | 'softmax' (--loss) train on a ranking loss of every positive against its own negatives
        clip_grad_norm = 0.0             # not in the reference (whose step has no clipping): X > 0 (--clip_grad_norm X) scales every step's gradient so that its global L2 norm is at most X, as torch.nn.utils.clip_grad_norm_ does; 0 = off
        negative_pool = 0                # not in the reference: M > 0 (--hard_negatives M) draws a pool of M random candidates per positive and trains on the random_negative_sample_size of them that the model scores highest; 0 = off
        filter_negatives = False         # not in the reference (whose negatives are uniform over the catalogue): True (--filter_negatives) draws every random negative outside the items the positive's user interacted with in training, the positive itself included
        popularity_power = 0.0           # not in the reference (whose negatives are uniform over the catalogue): A in (0, 1] (--popularity_negatives [A], a bare flag = 0.75) draws every random negative in proportion to its item's training frequency raised to A; 0 = off

    class Evaluation:
        extra_cutoffs = ()               # not in the reference (which reports @10 only): further cutoffs K in 11..128 (--cutoffs), HR / NDCG / MAP @K beside the @10 triple
        filter_seen = False              # not in the reference (which ranks the whole catalogue): True (--filter_seen) ranks every test log without the items its user interacted with in training, the log's own positives kept
        sampled_candidates = 0           # not in the reference: N > 0 (--eval_candidates N) ranks every test log among its own logged items plus N items drawn uniformly from the rest of the catalogue (the sampled-metrics protocol; not comparable with whole-catalogue metrics)
        candidate_seed = 0               # the seed of those draws: log i draws from numpy's default_rng([candidate_seed, i]), whatever the rank or the chunk it is evaluated in

    class Srrl:                          # the Srrl baseline (GlobalSettings.py:87-91)
        KG_loss = True                   # train the KG embeddings (srrl_steps KG steps per epoch) and feed them to the PS model through g_u / g_i
        uni_weight = False               # True: every positive weighs the same in the KG loss; False: sqrt(1 / frequency of its (user, query))
        regularization = 0               # != 0: adds the tables' squared norms to the REPORTED loss only (formed from .weight.data: no gradient)

    class Dataset:
        user_history_limit = 500

    class Debug:
        show_highorder_embedding_info = False
        _calculate_embedding_info = False
        _calculate_highorder_info = False
