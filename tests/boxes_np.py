"""Literal numpy / pandas restatement of the table half of the reference's src/error_boxes.py `plot_error` (and of
src/_defs/defs.py `quantile` / `iqr_interval`), the oracle of tests/test_gpu_error_boxes.py.  Stable argsort: the order this
package defines for ties."""
import collections

import numpy as np
import pandas as pd

EDGES = (.5, 1.5, 3.5, 7.5)


def quantile(n):
    def q_(x):
        return x.quantile(n)
    q_.__name__ = f'q_{n*100:.0f}'
    return q_


def iqr_interval(n, sign=1):
    def iqr(x):
        return x.quantile(.75) - x.quantile(.25)

    def iqr_interval_(x):
        return (x.quantile(n) + sign * iqr(x)).clip(x.min(), x.max())

    iqr_interval_.__name__ = f'q_{n*100:.0f}_iqr'
    return iqr_interval_


def _sliced(results, anchor_channel, edges):
    points = collections.OrderedDict([(k, np.asarray(x).flatten()) for k, x in results.items()])
    order = np.argsort(points[anchor_channel], kind="stable")
    points = collections.OrderedDict([(k, x[order]) for k, x in points.items()])
    anchor_edge_values = list(edges)
    anchor_edges = [np.argmin(points[anchor_channel] <= e) - 1 for e in anchor_edge_values]
    anchor_edges = [0] + anchor_edges + [len(points[anchor_channel])]
    anchor_edge_values = [0] + anchor_edge_values + [np.inf]
    for k, x in points.items():
        for j in range(len(anchor_edges) - 1):
            yield k, f'{anchor_edge_values[j]}-{anchor_edge_values[j+1]}', x[anchor_edges[j]:anchor_edges[j + 1]]


def table(results, anchor_channel, edges=EDGES):
    """plot_error's DataFrame, through pandas explode / groupby / agg as the reference builds it."""
    df = []
    for k, label, values in _sliced(results, anchor_channel, edges):
        df.append(pd.DataFrame([{'Type': k, 'edge_interval': label, 'values': values}]).explode('values'))
    df = pd.concat(df)
    df['values'] = df['values'].astype('float64')
    df = (
        df.groupby(['Type', 'edge_interval'])
        .agg({'values': [
            'min',
            iqr_interval(.25, sign=-1.5),
            quantile(.25),
            quantile(.5),
            quantile(.75),
            iqr_interval(.75, sign=1.5),
            'max',
        ]})
    )
    df.columns = [col[1] for col in df.columns.values]
    return df.reset_index().sort_values(['edge_interval', 'Type'])


def table_numpy(results, anchor_channel, edges=EDGES):
    """The same slices, the statistics by numpy directly (np.quantile 'linear' is what pandas' quantile calls): for arrays too large
    for explode's object rows."""
    rows = []
    for k, label, values in _sliced(results, anchor_channel, edges):
        s = values.astype(np.float64)
        if s.size == 0:
            rows.append({'Type': k, 'edge_interval': label, **{c: np.nan for c in
                         ('min', 'q_25_iqr', 'q_25', 'q_50', 'q_75', 'q_75_iqr', 'max')}})
            continue
        q25, q50, q75 = (np.quantile(s, q) for q in (.25, .5, .75))
        mn, mx = s.min(), s.max()
        rows.append({'Type': k, 'edge_interval': label, 'min': mn, 'q_25_iqr': (q25 + -1.5 * (q75 - q25)).clip(mn, mx), 'q_25': q25,
                     'q_50': q50, 'q_75': q75, 'q_75_iqr': (q75 + 1.5 * (q75 - q25)).clip(mn, mx), 'max': mx})
    df = pd.DataFrame(rows).sort_values(['Type', 'edge_interval']).reset_index(drop=True)
    return df.sort_values(['edge_interval', 'Type'])
