#!/usr/bin/env python
"""Summarise the debug timestamps of the fused hop-0 + hop-1 launch (TGMX_FUSED_TS=<prefix>: recency.hip writes <prefix>.0 .. .15,
one file per launch, the last 16 launches of a run).

    python tools/fused_ts_report.py <prefix> [--json out.json] [--groups 3] [--slots 7168]

Per launch: when the rider and commit workgroups end against the last lookup wave (us from the launch's first wave start), and the
hop-1 waves' lifetimes with the share of their seed (hop-0 pick), index (the rows' picks) and gather phases.  One-row hop-1 waves
carry their row s0 * k0 + j (word 6; older files carry none: the waves take the rows in output order, so it is derived): their lives
and start times are also split by seed group (--groups equal groups) and by quad of j, and the lookup waves resident at every
microsecond of the launch are counted against --slots wave slots."""
import argparse
import glob
import json

import numpy as np

MAGIC = 0x54474D5854530001
ROLES = {1: 'rider', 2: 'commit', 3: 'hop0', 4: 'hop1'}


def load(path):
    raw = np.fromfile(path, dtype=np.int64)
    assert raw[0] == MAGIC, f'{path}: not a fused-launch timestamp file'
    waves, side, commit, S0, k0, rows, khz = (int(v) for v in raw[1:8])
    rec = raw[8:].reshape(waves, 8)
    return {'side_blocks': side, 'commit_blocks': commit, 'S0': S0, 'k0': k0, 'rows_per_wave': rows, 'clock_khz': khz}, rec


def pct(a, q):
    return float(np.percentile(a, q)) if len(a) else None


def one(path, groups=3, slots=7168):
    hdr, rec = load(path)
    us = 1e3 / hdr['clock_khz']  # clock ticks -> us
    role = rec[:, 2] & 0xFF
    live = rec[:, 0] > 0
    t0 = rec[live, 0].min()
    start, end = (rec[:, 0] - t0) * us, (rec[:, 1] - t0) * us
    out = dict(hdr, file=path, launch_span_us=float(end[live].max()))
    for r, name in ROLES.items():
        sel = live & (role == r)
        if sel.any():
            out[f'{name}_waves'] = int(sel.sum())
            out[f'{name}_end_max_us'] = float(end[sel].max())
            out[f'{name}_life_avg_us'] = float((end[sel] - start[sel]).mean())
    look = live & ((role == 3) | (role == 4))
    out['last_lookup_end_us'] = float(end[look].max())
    if 'rider_end_max_us' in out:
        out['rider_ends_before_last_lookup_us'] = out['last_lookup_end_us'] - out['rider_end_max_us']
    h1 = live & (role == 4)
    life = end[h1] - start[h1]
    out['hop1_life_us'] = {'avg': float(life.mean()), 'p10': pct(life, 10), 'p50': pct(life, 50), 'p90': pct(life, 90), 'max': float(life.max())}
    if hdr['rows_per_wave'] > 0:  # the row-run schedule records its phases
        seed = (rec[h1, 3] - rec[h1, 0]) * us
        index = rec[h1, 4] * us
        gather = rec[h1, 5] * us
        rest = life - seed - index - gather
        tot = life.sum()
        out['hop1_phase_avg_us'] = {'seed': float(seed.mean()), 'index': float(index.mean()), 'gather': float(gather.mean()), 'other': float(rest.mean())}
        out['hop1_phase_share'] = {'seed': float(seed.sum() / tot), 'index': float(index.sum() / tot), 'gather': float(gather.sum() / tot),
                                   'other': float(rest.sum() / tot)}
    if hdr['rows_per_wave'] == 0:
        row = rec[h1, 6]
        if len(row) > 1 and not row.any():  # an older file: no row recorded, the waves took the rows in output order
            row = np.flatnonzero(h1) - hdr['S0'] - 4 * (hdr['side_blocks'] + hdr['commit_blocks'])
        s0, j = row // hdr['k0'], row % hdr['k0']
        st1 = start[h1]

        def split(key, n):
            return [{'waves': int((key == g).sum()), 'life_avg_us': float(life[key == g].mean()), 'life_p90_us': pct(life[key == g], 90),
                     'start_p50_us': pct(st1[key == g], 50), 'end_max_us': float(end[h1][key == g].max())} if (key == g).any() else None for g in range(n)]

        if groups > 0 and hdr['S0'] % groups == 0:
            out['hop1_by_group'] = split(s0 // (hdr['S0'] // groups), groups)
        out['hop1_by_quad'] = split(j // 4, (hdr['k0'] + 3) // 4)
    # lookup waves resident at every microsecond of the launch, against the wave slots of the device
    grid = np.arange(0.0, out['last_lookup_end_us'], 1.0)
    resident = [int(((start[look] <= t) & (end[look] > t)).sum()) for t in grid]
    out['resident_lookup_waves_by_us'] = resident
    out['slots'] = slots
    out['slots_in_use_avg'] = float(np.mean(resident) / slots) if resident else None
    # lookup waves resident over time: the launch's fill and drain
    out['hop1_start_p50_us'] = pct(start[h1], 50)
    out['hop1_start_p90_us'] = pct(start[h1], 90)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('prefix')
    p.add_argument('--json', default=None)
    p.add_argument('--groups', type=int, default=3, help='equal seed groups of the launch (src | dst | neg)')
    p.add_argument('--slots', type=int, default=7168, help='wave slots of the device at the kernel\'s occupancy (256 CUs x 4 SIMDs x 7)')
    args = p.parse_args()
    res = [one(f, args.groups, args.slots) for f in sorted(glob.glob(args.prefix + '.*')) if not f.endswith('.json')]
    keys = ['launch_span_us', 'rider_end_max_us', 'commit_end_max_us', 'last_lookup_end_us', 'rider_ends_before_last_lookup_us']
    summary = {'launches': len(res), 'rows_per_wave': res[0]['rows_per_wave'] if res else None}
    for k in keys:
        v = [r[k] for r in res if k in r]
        if v:
            summary[k] = {'avg': float(np.mean(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}
    for k in ('avg', 'p10', 'p50', 'p90', 'max'):
        summary.setdefault('hop1_life_us', {})[k] = float(np.mean([r['hop1_life_us'][k] for r in res]))
    for key in ('hop1_by_group', 'hop1_by_quad'):
        if res and all(key in r and None not in r[key] for r in res):
            summary[key] = [{f: float(np.mean([r[key][g][f] for r in res])) for f in res[0][key][g]} for g in range(len(res[0][key]))]
    if res:
        summary['slots_in_use_avg'] = float(np.mean([r['slots_in_use_avg'] for r in res]))
        n = min(len(r['resident_lookup_waves_by_us']) for r in res)
        summary['slots_in_use_by_us'] = [round(float(np.mean([r['resident_lookup_waves_by_us'][t] for r in res])) / args.slots, 3) for t in range(n)]
    if res and 'hop1_phase_share' in res[0]:
        for k in ('seed', 'index', 'gather', 'other'):
            summary.setdefault('hop1_phase_avg_us', {})[k] = float(np.mean([r['hop1_phase_avg_us'][k] for r in res]))
            summary.setdefault('hop1_phase_share', {})[k] = float(np.mean([r['hop1_phase_share'][k] for r in res]))
    print(json.dumps(summary, indent=1))
    if args.json:
        json.dump({'summary': summary, 'launches': res}, open(args.json, 'w'), indent=1)


if __name__ == '__main__':
    main()
