"""dev tool: the kernel table of profiles/grad_rows_bf16_kernel_stats.txt -- two tools/rocpd_stats.py summaries (rocprofv3 --kernel-trace
--stats of `bench.py --gpus 1 --steps 8 --warmup 3` with ES_GRAD_ROWS_BF16=0 and =1, no counters) and a launch census (every call of the
entry points the switch touches, with its integer arguments, recorded through engine.call / hip.try_call in a run of its own, as
{"steps": backward passes seen, "launches": [[name, args...], ...]}) -> per kernel family: calls and ms per step, the bytes the family's
launches must move per step (from the census shapes) and the GB/s reached.

  python tools/grad_rows_bf16_table.py STATS_OFF STATS_ON CENSUS_JSON [STEPS_IN_CENSUS, where the census does not carry its count]"""
import json
import re
import sys


def stats(path):
    out = {}
    for ln in open(path):
        m = re.match(r'^(.*?)\s+(\d+)\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)\s*$', ln)
        if m:
            out[m.group(1).strip()] = (int(m.group(2)), float(m.group(3)))
    return out


def family(st, pred):
    calls = sum(c for k, (c, _) in st.items() if pred(k))
    ms = sum(t for k, (_, t) in st.items() if pred(k))
    return calls, ms


def census_bytes(census, steps):
    """bytes per step each family must move, switch ON, and what the same launches moved with f32 rows (OFF)"""
    per = {}

    def add(fam, on, off):
        e = per.setdefault(fam, [0, 0])
        e[0] += on / steps
        e[1] += off / steps
    for r in census:
        fn, a = r[0], r[1:]
        if fn == 'es_affine_act_bwd_yh_xh':                 # dy f32 + y bf16 in; bf16 rows (+ f32 dres) out, dres re-read when accumulated
            e = a[3] * a[4]
            res = (4 * e if a[7] else 0) + (4 * e if a[7] and a[8] else 0)
            add('join', e * (4 + 2 + 2) + res, e * (4 + 2 + 4) + res)
        elif fn == 'es_affine_act_bwd_yh_xh2':              # two bf16 matrices out, no dres; off: join with dres + the act = 0 launch on it
            e = a[4] * a[5]
            add('join', e * (4 + 2 + 2 + 2), e * (4 + 2 + 4 + 4) + e * (4 + 4))
        elif fn == 'es_affine_act_bwd_yh':
            e = a[3] * a[4]
            res = (4 * e if a[8] else 0) + (4 * e if a[8] and a[9] else 0)
            b = e * (4 + 2 + (4 if a[6] else 0)) + res
            add('join', b, b)
        elif fn == 'es_spconv_fwd_bf16_io' and a[15] == 3 and a[7] == 1:      # gated K = 1 data gradient: G in, gate bf16 in, f32 out
            n, red, out = a[5], a[8], a[9]
            add('row GEMMs (MB: gated K=1 dgrads)', n * red * (2 if a[1] else 4) + n * out * (2 + 4), n * red * 4 + n * out * (2 + 4))
        elif fn == 'es_spconv_wgrad_bf16_src' and a[9] == 1 and a[6] == 0:    # identity-map K = 1 weight gradient
            n, cin, cout = a[7], a[10], a[11]
            add('map wgrad <1,*> (MB: K=1 launches)', n * cin * (2 if a[1] else 4) + n * cout * (2 if a[4] else 4), n * cin * (2 if a[1] else 4) + n * cout * 4)
        elif fn == 'es_rows_wgrad1_bf16':
            n, cin, cout = a[4], a[5], a[6]
            add('k_rows_wgrad1', n * cin * 2 + n * cout * (2 if a[8] & 2 else 4), n * cin * 2 + n * cout * 4)
        elif fn == 'es_norm_bwd':                           # apply pass: dz + x in, bf16 and / or f32 rows out (the statistics pass is separate)
            n, C, nseg, lean, shadow = a[6], a[7], a[9], a[17] == 0, a[20] != 0
            fam = 'k_norm_bwd_cb' if (nseg == 1 and n <= 4096 and C % 16 == 0) else 'k_norm_bwd_apply4'
            rd = n * C * 8 * (2 if fam == 'k_norm_bwd_cb' else 1) + (n * C * 4 if fam == 'k_norm_bwd_cb' else 0)   # cb: dy, y / x twice + dz store
            add(fam, rd + n * C * ((0 if lean else 4) + (2 if shadow else 0)), rd + n * C * (4 + (2 if shadow else 0)))
        elif fn == 'es_cast_rows_bf16':
            add('k_cast_rows8', a[2] * a[3] * 6, a[2] * a[3] * 6)
        elif fn == 'es_img_dgrad1_s2_bf16':
            n = a[3] * (a[4] // 2) * (a[5] // 2)             # gradient rows in, the even pixels' rows out (+ zeros to the other three)
            add('k_img_dgrad1_s2', n * a[6] * (2 if a[10] & 2 else 4) + 4 * n * a[7] * 4, n * a[6] * 4 + 4 * n * a[7] * 4)
    return per


def main(off_path, on_path, census_path, census_steps=None):
    off, on = stats(off_path), stats(on_path)
    steps = family(off, lambda k: k.startswith('k_norm_final('))[0]            # one clip-norm launch per train step
    census = json.load(open(census_path))
    csteps = int(census_steps) if census_steps else census['steps']
    assert csteps > 0, 'the census carries no step count: give STEPS_IN_CENSUS'
    by = census_bytes(census['launches'], csteps)
    fams = [('join', lambda k: k.startswith('k_affine_act_bwd4_yh')),
            # (a trace cannot tell the gated data gradients from the forward row GEMMs of the same instantiation, nor the K = 1 weight
            # gradients from the K = 27 ones: calls and ms are the whole kernel family's, MB the touched launches' alone -- no rate is given)
            ('row GEMMs (MB: gated K=1 dgrads)', lambda k: 'k_rowgemm2_bf16<' in k and ', false, true>' in k),
            ('map wgrad <1,*> (MB: K=1 launches)', lambda k: 'k_spconv_wgrad_bf16<1, ' in k or 'k_spconv_wgrad_bf16_big<1, ' in k),
            ('k_rows_wgrad1', lambda k: 'k_rows_wgrad1<' in k),
            ('k_img_dgrad1_s2', lambda k: 'k_img_dgrad1_s2' in k),
            ('k_cast_rows8', lambda k: k.startswith('k_cast_rows8')),
            ('k_norm_bwd_apply4', lambda k: k.startswith('k_norm_bwd_apply4')),
            ('k_norm_bwd_cb', lambda k: k.startswith('k_norm_bwd_cb'))]
    print(f'{steps} train steps per trace; census of {csteps} steps; calls and ms are per step; MB = bytes the launches must move per step')
    print(f'{"family":36s} | {"calls":>6s} {"ms":>7s} {"MB":>8s} {"GB/s":>7s} | {"calls":>6s} {"ms":>7s} {"MB":>8s} {"GB/s":>7s} | {"ms saved":>8s}')
    print(f'{"":36s} | {"switch off":>31s} | {"switch on":>31s} |')
    tot = 0.0
    for name, pred in fams:
        (c0, t0), (c1, t1) = family(off, pred), family(on, pred)
        b1, b0 = by.get(name, [0, 0])
        t0, t1 = t0 / steps, t1 / steps
        rate = '(MB:' not in name
        g0 = f'{b0 / t0 / 1e6:7.0f}' if t0 and b0 and rate else '    n/a'
        g1 = f'{b1 / t1 / 1e6:7.0f}' if t1 and b1 and rate else '    n/a'
        tot += t0 - t1
        print(f'{name:36s} | {c0 / steps:6.1f} {t0:7.3f} {b0 / 1e6:8.1f} {g0} | {c1 / steps:6.1f} {t1:7.3f} {b1 / 1e6:8.1f} {g1} | {t0 - t1:8.3f}')
    def total(path):
        return float(re.search(r'total kernel time ([\d.]+) ms', open(path).read()).group(1))
    k0, k1 = total(off_path) / steps, total(on_path) / steps
    print(f'sum of the rows: {tot:.3f} ms per step; kernel time of the whole process: {k0:.3f} -> {k1:.3f} ms per step')


if __name__ == '__main__':
    main(*sys.argv[1:])
