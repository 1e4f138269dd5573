"""Shared data of tests/test_cpu_rows_hint.py and tests/test_gpu_rows_hint.py: a small interaction store on which every
train and eval batch of the batchers holds fewer valid context positions than B x L (so each one packs), for world 1 and 2."""
import numpy as np

N, C, U = 200, 3, 150
L, P, E, B = 24, 2, 2, 16
BUCKET = 64


def make_data():
    g = np.random.default_rng(5)
    lens = g.integers(9, 19, U)
    tags = g.random((N, C)) < 0.45
    tags[np.arange(N), g.integers(0, C, N)] = True
    tags[0] = False
    user_seq = [[]] + [g.integers(1, N, int(n)).tolist() for n in lens]
    train_len = [0] + [len(s) - 4 for s in user_seq[1:]]            # train prefix | 2 validation items | 2 test items
    return user_seq, train_len, tags


def config_dict(**kw):
    c = dict(MAX_ITEM_LIST_LENGTH=L, pred_len=P, eval_pred_len=E, loss='prior', neg_sample_by_cat=True, category_by='item',
             neg_sample_mix_ratio=0, pad_random_sample=True, num_negatives=64, train_batch_size=B, eval_batch_size=B,
             eval_num_cats=C, outlier_user_metrics=None)
    c.update(kw)
    return c
