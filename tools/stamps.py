"""Diagnostic: per-wave phase times of the fused kernel from the PRF_STAMPS build (libprf_stamps.so).
Usage (GPU box): PRF_LIB=colab-repeat-finder_amd/libprf_stamps.so PRF_STAMPS_OUT=/tmp/st.bin python tools/stamps.py [length]"""
import os, re, sys
import numpy as np
sys.path.insert(0, 'colab-repeat-finder_amd'); sys.path.insert(0, '.')
import prf_native, synth
L = int(sys.argv[1]) if len(sys.argv) > 1 else 50_818_468
ctx = prf_native.Context(0)
if len(sys.argv) > 2 and sys.argv[2] == 'standin2':   # the default bench workload's recipe, generated on the device
    g = ctx.standin([L], [1], 50)
else:
    seq = synth.chr_standin(length=L, seed=22, n_head=10_510_000 if L > 2e7 else L // 10, n_tail=10_000).tobytes()
    g = ctx.load([seq], 50)
for _ in range(3):
    g.scan(1, 50, 3, 9, fetch=False)
_, st = g.scan(1, 50, 3, 9, fetch=False)
print('kernel ms', st.phase1_ms)
st_ms_global = st.phase1_ms
# words per (launch slot, wave) of the stamp record: the kernel's own constant
SLOTS = int(re.search(r'#define PRF_STAMP_SLOTS (\d+)', open('colab-repeat-finder_amd/csrc/scan_vertical.h').read()).group(1))
d = np.fromfile(os.environ['PRF_STAMPS_OUT'], dtype=np.uint64).reshape(-1, 4, SLOTS).astype(np.int64)
t0 = d[:, :, 0].min()
names = ['stage', 'bar1', 'scan', 'bar2', 'verify', 'bar3', 'rows']
for w in range(4):
    seg = [np.median(d[:, w, i + 1] - d[:, w, i]) for i in range(7)]
    print('wave', w, ' '.join(f'{n}={int(v)}' for n, v in zip(names, seg)), 'total', int(np.median(d[:, w, 7] - d[:, w, 0])))
print('WG start spread (cycles): min', 0, 'median', int(np.median(d[:, 0, 0] - t0)), 'max', int((d[:, 0, 0] - t0).max()))
print('WG end   (cycles): median', int(np.median(d[:, :, 7].max(axis=1) - t0)), 'max', int((d[:, :, 7].max(axis=1) - t0).max()))
tot = (d[:, :, 7].max(axis=1) - d[:, :, 0].min(axis=1))
print('WG total cycles: p50', int(np.percentile(tot, 50)), 'p90', int(np.percentile(tot, 90)), 'p99', int(np.percentile(tot, 99)), 'max', int(tot.max()), 'argmax', int(tot.argmax()), 'of', len(tot))
print('last 4 WGs (mixed tiles are last):', tot[-4:])
ends = np.sort(d[:, :, 7].max(axis=1) - t0)
print('WG end percentiles (cycles from first start): p10 %d p50 %d p90 %d p99 %d max %d' % tuple(int(np.percentile(ends, q)) for q in (10, 50, 90, 99, 100)))
order = np.argsort(tot)[-6:]
for i in order:
    print('slow WG', int(i), 'total', int(tot[i]), 'phases w0', [int(d[i, 0, j + 1] - d[i, 0, j]) for j in range(6)])

# per-task durations (cycles, median over workgroups): slot 8+i = start of the wave's i-th task (the first four), slot 17 = end of
# its last task, in front of the arrival atomic
for w in range(4):
    starts = [d[:, w, 8 + i] for i in range(4)]
    out = []
    for i in range(4):
        if np.median(starts[i]) == 0: break
        nxt = starts[i + 1] if i + 1 < 4 and np.median(starts[i + 1]) != 0 else d[:, w, 17]
        out.append(int(np.median(nxt - starts[i])))
    print('wave', w, 'task cycles', out, 'sum', sum(out), '; bar1 to first task', int(np.median(d[:, w, 8] - d[:, w, 2])),
          '; last task to stamp 3', int(np.median(d[:, w, 3] - d[:, w, 17])), '; scan (stamp 2 to 17)', int(np.median(d[:, w, 17] - d[:, w, 2])))

# The hand-over from the scan to the verification.  Clock: cycles from the tile's stamp 0 (the earliest wave's).  Slot 17 = a
# wave's arrival (end of its last task), 18 = its arrival order, 3 = arrival atomic back and window loads issued, 20 = the wave's
# window loads are in registers (the stamps build waits for them in front of the first barrier), 19 = behind the first barrier,
# 21 = its window stores are issued, 22 = pad loop and counters done (in front of the second barrier), 4 = behind the second
# barrier (verify start).
z = d[:, :, 0].min(axis=1)
clk = lambda s: d[:, :, s] - z[:, None]
print('arrival clock by wave:', [int(np.median(clk(17)[:, w])) for w in range(4)], ' verify start', int(np.median(clk(4).max(axis=1))))
by_order = lambda s: np.stack([np.where(d[:, :, 18] == o, clk(s), 0).sum(axis=1) for o in range(4)], axis=1)
valid = np.all(np.sort(d[:, :, 18], axis=1) == np.arange(4), axis=1)
print('tiles whose four waves hold the orders 0..3:', int(valid.sum()), 'of', len(valid))
for s, name in ((17, 'arrival (end of last task)'), (3, 'atomic back, loads issued'), (20, 'loads in registers'), (19, 'behind the first barrier'),
                (21, 'window stores issued'), (22, 'pad loop and counters done'), (4, 'behind the second barrier')):
    print('  %-28s by arrival order: %s' % (name, [int(np.median(by_order(s)[valid, o])) for o in range(4)]))
o17, o3, o19, o20, o21, o22, o4 = (by_order(s)[valid] for s in (17, 3, 19, 20, 21, 22, 4))
pct = lambda v: (int(np.median(v)), int(np.percentile(v, 10)), int(np.percentile(v, 90)))
print('W (arrival of the 2nd wave to its loads being in registers): median %d p10 %d p90 %d; of that from the issue of the loads %d; 1st wave: W %d, from the issue %d' % (
    *pct(o20[:, 1] - o17[:, 1]), int(np.median(o20[:, 1] - o3[:, 1])), int(np.median(o20[:, 0] - o17[:, 0])), int(np.median(o20[:, 0] - o3[:, 0]))))
fixed = o3[:, 3] - o17[:, 3]
print('fixed code behind the last arrival (its arrival to its stamp 3): median %d p10 %d p90 %d; to the barrier opening %d' % (*pct(fixed), int(np.median(o19.max(axis=1) - o17[:, 3]))))
print("W' = W - that fixed code: median %d p10 %d p90 %d" % pct((o20[:, 1] - o17[:, 1]) - fixed))
late = np.maximum(o20[:, 0], o20[:, 1]) - o3[:, 3]
print('the later of the two loading waves has its data %d cycles (median; p10 %d p90 %d) after the last wave is ready for the barrier; share of tiles where that is later %.3f' % (*pct(late), float((late > 0).mean())))
print('a4 - a2 (arrivals) median %d; a2 + W\' - a4 median %d' % (int(np.median(o17[:, 3] - o17[:, 1])), int(np.median(o20[:, 1] - fixed - o17[:, 3]))))
print('between the barriers, by arrival order: stores %s, pad loop and counters %s, wait at the second barrier %s; barrier to barrier %d' % (
    [int(np.median(o21[:, o] - o19[:, o])) for o in range(4)], [int(np.median(o22[:, o] - o21[:, o])) for o in range(4)],
    [int(np.median(o4[:, o] - o22[:, o])) for o in range(4)], int(np.median(o4.max(axis=1) - o19.max(axis=1)))))

nf = d[:, 0, 23] & 0xFFFFFFFF; nr = d[:, 0, 23] >> 32
print('flags per tile: mean %.1f p10 %d p50 %d p90 %d p99 %d max %d; share <=64 %.3f <=128 %.3f <=192 %.3f <=256 %.3f' % (
    nf.mean(), *[int(np.percentile(nf, q)) for q in (10, 50, 90, 99, 100)], *[(nf <= c).mean() for c in (64, 128, 192, 256)]))
print('records per tile: mean %.1f p10 %d p50 %d p90 %d p99 %d max %d; share <=64 %.3f <=128 %.3f <=192 %.3f' % (
    nr.mean(), *[int(np.percentile(nr, q)) for q in (10, 50, 90, 99, 100)], *[(nr <= c).mean() for c in (64, 128, 192)]))
import collections
print('joint (ceil(flags/64), ceil(recs/64)) shares:', sorted(((k, round(v / len(nf), 3)) for k, v in collections.Counter(zip(((nf + 63) // 64).tolist(), ((nr + 63) // 64).tolist())).items()), key=lambda kv: -kv[1])[:12])
for w in range(4):
    # (stamp 14: the flag waves 0, 1 set it behind the flags, the record waves 2, 3 between their stages A and B)
    print('wave', w, ('verify: flags part %d, boundary part %d' if w < 2 else 'verify: records stage A %d, stage B %d') % (
        int(np.median(d[:, w, 14] - d[:, w, 4])), int(np.median(d[:, w, 5] - d[:, w, 14]))))
for w in range(4):
    # slot 15: [21:0] inside the exact-task functions, [42:22] in push_flags, [63:43] in the group tasks' pushes (sums over the wave's tasks)
    body, pf, pg = d[:, w, 15] & 0x3FFFFF, (d[:, w, 15] >> 22) & 0x1FFFFF, (d[:, w, 15] >> 43) & 0x1FFFFF
    print('wave', w, 'cycles inside the exact-task functions (sum over the wave\'s exact tasks): median', int(np.median(body)))
    print('wave', w, 'cycles in pushes: exact/coarse tasks median %d mean %.0f, group tasks median %d mean %.0f; both, share of the wave\'s tile time %.3f' % (
        int(np.median(pf)), pf.mean(), int(np.median(pg)), pg.mean(), np.median((pf + pg) / np.maximum(1, d[:, w, 7] - d[:, w, 0]))))

# slot 16: cycles inside the rows phase's rank loop (key reads, compares, DPP adds; summed over the passes of a tile)
for w in range(4):
    rk = d[:, w, 16]
    print('wave', w, 'rank loop cycles: median %d mean %.0f p10 %d p90 %d; share of the rows phase %.3f, of the wave\'s tile time %.4f' % (
        int(np.median(rk)), rk.mean(), int(np.percentile(rk, 10)), int(np.percentile(rk, 90)),
        np.median(rk / np.maximum(1, d[:, w, 7] - d[:, w, 6])), np.median(rk / np.maximum(1, d[:, w, 7] - d[:, w, 0]))))

# slot utilisation from the chip-wide 100 MHz counter (slots 12 / 13 = workgroup start / end)
rs = d[:, :, 12].min(axis=1); re = d[:, :, 13].max(axis=1)
span = re.max() - rs.min()
print('kernel span on the 100 MHz counter: %.1f us; workgroup time: p50 %.2f us; slot utilisation (256 CUs x 4): %.3f' % (
    span / 100.0, np.median(re - rs) / 100.0, (re - rs).sum() / (span * 1024.0)))
print('core cycles per 10 ns tick (p50 over workgroups): %.2f' % np.median((d[:, 0, 7] - d[:, 0, 0]) / np.maximum(1, d[:, 0, 13] - d[:, 0, 12])))
# how many workgroups are resident over time (per 5 us bucket)
edges = np.arange(rs.min(), re.max() + 500, 500)
res = [(int(((rs < e + 500) & (re > e)).sum())) for e in edges[:-1]]
print('resident workgroups per 5 us bucket:', res[:8], '...', res[len(res)//2 - 2: len(res)//2 + 2], '...', res[-6:])
