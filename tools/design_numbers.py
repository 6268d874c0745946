"""Fills the @@name@@ fields of a DESIGN.md template with the numbers of a profile collection (tools/collect_profiles.sh):
    python tools/design_numbers.py tools/DESIGN.template.md profiles > DESIGN.md
Every field is read from the file DESIGN.md names next to it; a field the files do not yield stays visible as @@name@@."""
import csv
import json
import os
import re
import sys


def stats(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(l for l in f if not l.startswith('#')):
            rows[r['kernel']] = r
    return rows


def main(template, d):
    v = {}
    P = lambda n: os.path.join(d, n)
    rb_path = P('run_bench.json')
    ba_path = P('ba_bench.json')
    bench_train_5000x64 = [r for r in (json.loads(l) for l in open(P('r06_bench_train.json')) if l.strip())
                           if r.get('rays') == 5000 and r.get('samples_per_ray') == 64][0]['ms_per_iter_fused_graph']
    # the Mesher's tail: host methods against the device path (tools/mesh_bench.py)
    mt = json.load(open(P('mesh_tail_bench.json')))['by_resolution']

    def thousands(n):
        return f'{n:,}'.replace(',', ' ')
    legs = [('seen mask, 4 keyframes (`point_masks` / `seen_mask`)', 'seen_mask_4_keyframes'),
            ('seen mask, 300 poses, `get_mask_use_all_frames`', 'seen_mask_300_poses_all_frames'),
            ('culling (`Mesher.clean` / `mesh.clean_components`)', 'clean'),
            ('vertex merge, 1 % planted duplicates', 'merge_coincident'),
            ('whole tail: marching-cubes output → arrays for `write_ply`', 'whole_tail')]
    rows = []
    for name, key in legs:
        cells = []
        for res in ('256', '512'):
            h, dv = mt[res]['tail'][key]['host'], mt[res]['tail'][key]['device']
            cells.append('%.1f (%.1f, %.1f) | %.2f (%.2f, %.2f)' % (h['median_ms'], h['min_ms'], h['spread_ms'], dv['median_ms'], dv['min_ms'],
                                                                    dv['spread_ms']))
        rows.append('| %s | %s |' % (name, ' | '.join(cells)))
    v['mt_table'] = '\n'.join(rows)
    for res in ('256', '512'):
        r = mt[res]
        v['mt_v' + res], v['mt_f' + res] = thousands(r['verts']), thousands(r['faces'])
        v['mt_kv' + res], v['mt_kf' + res] = thousands(r['tail']['kept_verts']), thousands(r['tail']['kept_faces'])
        v['mt_h' + res] = '%.1f' % r['tail']['whole_tail']['host']['median_ms']
        v['mt_d' + res] = '%.2f' % r['tail']['whole_tail']['device']['median_ms']
        v['mt_bound' + res] = '%.0f' % r['get_bound_planes_host_ms']
    rep = json.load(open(P('mesh_tail_bench_256_repeat.json')))['by_resolution']['256']['tail']
    v['mt_rep_lo'] = '%.2f' % min(rep['clean']['device']['all_ms'])
    v['mt_rep_hi'] = '%.2f' % max(rep['clean']['device']['all_ms'])
    v['mt_rep_tail'] = '%.2f' % rep['whole_tail']['device']['median_ms']
    v['mt_getmesh512'] = '%.0f' % (mt['512']['get_mesh_total']['median_s'] * 1e3)
    # the mesh bound: host route against device route (tools/bound_bench.py) and the kernel trace of the device route
    mb = json.load(open(P('mesh_bound_bench.json')))
    cell = lambda s, f='%.1f': (f + ' (' + f + ', ' + f + ')') % (s['median_ms'], s['min_ms'], s['spread_ms'])
    rows = []
    for name, w in sorted(mb['workloads'].items()):
        rows.append('| (%s) %d × %d × %d | %s | %s | %s | %.0f× | %d | %s |' % (
            name, w['keyframes'], w['frame'][0], w['frame'][1], thousands(w['points']), cell(w['host']), cell(w['device'], '%.2f'),
            w['host_over_device_median'], w['rounds'], ', '.join(thousands(n) for n in w['survivors_per_round'])))
        v['mb_qhull_' + name] = '%.1f' % sum(w['qhull_ms_per_round'])
        v['mb_dict_' + name] = '%.1f' % w['device_from_keyframe_dict']['median_ms']
        v['mb_vertices_' + name] = str(w['vertices'])
    v['mb_table'] = '\n'.join(rows)
    ds = sorted(mb['workloads']['a']['by_directions'], key=int)
    v['mb_d_table'] = '\n'.join('| %s | %s |' % (D, ' | '.join('%.2f, %s' % (w['by_directions'][D]['depth_hull']['median_ms'],
                                                                              thousands(w['by_directions'][D]['survivors_per_round'][0]))
                                                               for _, w in sorted(mb['workloads'].items()))) for D in ds)
    v['mb_D'] = str(mb['D'])
    v['mb_single'] = 'wins' if mb['single_routing'] else 'does NOT win'
    for res in ('256', '512'):
        g = mb['get_mesh'][res]
        v['mb_gm' + res] = '%.1f' % g['get_mesh']['median_ms']
        v['mb_gmb' + res] = '%.2f' % g['bound_planes']['median_ms']
        v['mb_gmh' + res] = '%.0f' % g['get_bound_planes_host']['median_ms']
        v['mb_share' + res] = '%.1f' % (100 * g['bound_share_of_get_mesh'])
    ks = stats(P('mesh_bound_kernels.csv'))
    # (the recorded trace is of the build that introduced the bound: its tile scan ran as k_mcl_tile_scan, today's k_tile_scan)
    for name in ('k_bnd_support(', 'k_bnd_support_fold', 'k_bnd_flag', 'k_bnd_emit', 'k_bnd_far<0>', 'k_bnd_far<1>', 'k_mcl_tile_scan'):
        r = next((r for k, r in ks.items() if name in k), None)
        if r:
            key = 'mbk_' + re.sub(r'\W', '', name)
            v[key + '_max'] = '%.0f' % float(r['max_us']); v[key + '_avg'] = '%.1f' % float(r['avg_us']); v[key + '_calls'] = r['calls']
    wb = mb['workloads']['b']
    n_ids = wb['keyframes'] * (wb['frame'][0] * wb['frame'][1] + 1)
    v['mbk_ids'] = thousands(n_ids); v['mbk_F'] = str(wb['planes_per_round'][0])
    v['mbk_hbm_us'] = '%.0f' % (4.0 * n_ids / 6.29e12 * 1e6)            # the depth block once at the measured HBM rate
    if 'mbk_k_bnd_flag_max' in v:
        v['mbk_flag_tops'] = '%.1f' % (7.0 * n_ids * wb['planes_per_round'][0] / (float(v['mbk_k_bnd_flag_max']) * 1e-6) / 1e12)
    if 'mbk_k_bnd_support_max' in v:
        v['mbk_support_tops'] = '%.1f' % (5.0 * n_ids * mb['D'] / (float(v['mbk_k_bnd_support_max']) * 1e-6) / 1e12)
    # frame ingestion: host chain against device route (tools/ingest_bench.py)
    ib = json.load(open(P('ingest_bench.json')))
    v['ing_cpus'], v['ing_threads'] = str(ib['host']['cpus']), str(ib['host']['torch_threads'])
    v['ing_reps'], v['ing_iters'] = str(ib['reps']), str(ib['iters'])
    ik = {n: stats(P('ingest_kernels_%d.csv' % n)) for n in (1, ib['frames_per_batch'])}
    v['ing_hbm'] = '6.3'
    rows, lrows = [], []
    for name, g in sorted(ib['geometries'].items()):
        shape = '%s: %d × %d → %d × %d' % (name, g['color'][0], g['color'][1], g['out'][0], g['out'][1])
        rows.append('| %s | %s | %s | %s | %.0f× | %s → %s |' % (
            shape, cell(g['host_chain'], '%.2f'), cell(g['device_1_frame'], '%.3f'), cell(g['device_8_frames_per_frame'], '%.3f'),
            g['host_over_device_median'], thousands(g['upload_bytes_host_route']), thousands(g['upload_bytes_device_route'])))
        la = g['launch']
        k1, k8 = (next(r for k, r in ik[n].items() if 'k_ingest<%d, float>' % (0 if g['color'] == g['depth'] else 1) in k)
                  for n in (1, ib['frames_per_batch']))
        lrows.append('| %s | %s | %.1f µs | %.1f µs | %.1f µs | %.1f µs | %.1f TB/s |' % (
            shape, thousands(la['bytes_per_frame']), la['ms_1_frame'] * 1e3, la['ms_per_frame_of_8'] * 1e3, float(k1['avg_us']), float(k8['avg_us']),
            ib['frames_per_batch'] * la['bytes_per_frame'] / (float(k8['avg_us']) * 1e-6) / 1e12))
    v['ing_table'], v['ing_launch_table'] = '\n'.join(rows), '\n'.join(lrows)
    tum = ib['tum']                                             # lens undistortion at TUM RGB-D's frame (--tum-only)
    v['ing_tum_out'] = '%d × %d' % tuple(tum['out'])
    v['ing_tum_reps'], v['ing_tum_iters'] = str(tum['reps']), str(tum['iters'])
    v['ing_tum_host'] = cell(tum['host_statement'], '%.2f')
    for key, field in (('dev1', 'device_1_frame'), ('dev8', 'device_8_frames_per_frame'), ('plain1', 'plain_device_1_frame'),
                       ('plain8', 'plain_device_8_frames_per_frame')):
        v['ing_tum_' + key] = cell(tum[field], '%.3f')
    for key, kind in (('l', 'undistort'), ('pl', 'plain')):
        v['ing_tum_%s1' % key] = '%.1f' % (tum['launch'][kind]['ms_1_frame'] * 1e3)
        v['ing_tum_%s8' % key] = '%.1f' % (tum['launch'][kind]['ms_8_frames'] * 1e3)
    v['ing_tum_ratio8'] = '%.2f' % tum['launch_undistort_over_plain_8_frames']
    v['ing_tum_map_ms'], v['ing_tum_map_numpy_ms'] = '%.1f' % tum['map_library_ms'], '%.0f' % tum['map_numpy_ms']
    # the Visualizer after render_img: host chain against device route (tools/vis_bench.py) and the per-configuration kernel trace
    vb = json.load(open(P('vis_bench.json')))
    v['vis_cpus'], v['vis_threads'] = str(vb['host']['cpus']), str(vb['host']['torch_threads'])
    v['vis_reps'], v['vis_iters'], v['vis_mpl'] = str(vb['reps']), str(vb['iters']), str(vb['host']['matplotlib'])
    with open(P('vis_kernels.csv')) as f:
        vk = {(r['frame'], r['stride'], r['kernel']): r for r in csv.DictReader(l for l in f if not l.startswith('#'))}
    rows, krows = [], []
    for name, g in sorted(vb['frames'].items()):
        shape = '%s: %d × %d' % (name, g['frame'][0], g['frame'][1])
        s1, s2 = g['by_stride']['1'], g['by_stride']['2']
        fig = cell(g['matplotlib_figure'], '%.0f') if g['matplotlib_figure'] else 'no matplotlib'
        rows.append('| %s | %s | %s | %s | %s | %.0f× | %.0f× | %s |' % (
            shape, cell(g['host_chain'], '%.2f'), cell(g['host_downloads_alone'], '%.2f'), cell(s1['device'], '%.3f'), cell(s2['device'], '%.3f'),
            s1['host_over_device_median'], s1['host_numpy_over_device_median'], fig))
        v['vis_numpy_' + name] = '%.1f' % (g['host_chain']['median_ms'] - g['host_downloads_alone']['median_ms'])
        for st, r in sorted(g['by_stride'].items()):
            kr, kp = vk[(name, st, 'k_vis_reduce')], vk[(name, st, 'k_vis_panels')]
            krows.append('| %s, stride %s | %d × %d | %s | %s | %.1f µs | %.1f (%.1f) | %.1f (%.1f) |' % (
                shape, st, r['canvas'][0], r['canvas'][1], thousands(g['input_bytes']), thousands(r['canvas_bytes']), r['launches_ms'] * 1e3,
                float(kr['avg_us']), float(kr['max_us']), float(kp['avg_us']), float(kp['max_us'])))
            v['vis_dev_%s%s' % (name, st)] = '%.2f' % r['device']['median_ms']
    v['vis_table'], v['vis_kernel_table'] = '\n'.join(rows), '\n'.join(krows)
    g = vb['frames']['replica']
    kp, kr = vk[('replica', '1', 'k_vis_panels')], vk[('replica', '1', 'k_vis_reduce')]
    moved = g['input_bytes'] + g['by_stride']['1']['canvas_bytes']
    v['vis_panels_replica1'] = '%.0f' % float(kp['avg_us'])
    v['vis_mb_replica1'] = '%.0f' % (moved / 1e6)
    v['vis_tbps_replica1'] = '%.1f' % (moved / (float(kp['avg_us']) * 1e-6) / 1e12)
    v['vis_launch_share_replica1'] = '%.0f' % (100 * (float(kp['avg_us']) + float(kr['avg_us'])) * 1e-3 / g['by_stride']['1']['device']['median_ms'])
    # rendering metrics of a run: host route against device route (tools/render_eval_bench.py) and the kernel trace
    rb = json.load(open(P('render_eval_bench.json')))
    v['re_cpus'], v['re_threads'] = str(rb['host']['cpus']), str(rb['host']['torch_threads'])
    v['re_numpy'], v['re_scipy'] = rb['host']['numpy'], rb['host']['scipy']
    v['re_reps'], v['re_iters'] = str(rb['reps']), str(rb['iters'])
    with open(P('render_eval_kernels.csv')) as f:
        rk = {(r['frame'], r['kernel']): r for r in csv.DictReader(l for l in f if not l.startswith('#'))}
    rows, prows, brows = [], [], []
    for name, g in sorted(rb['frames'].items()):
        nf = g['frames_per_table']
        many = g['device_%d_frames_per_frame' % nf]
        shape = '%s: %d × %d' % (name, g['frame'][0], g['frame'][1])
        rows.append('| %s | %s | %s | %s | %s | %.0f×, %.0f× | %s |' % (
            shape, cell(g['host_scipy'], '%.1f'), cell(g['host_downloads_alone'], '%.2f'), cell(g['device_1_frame'], '%.3f'), cell(many, '%.3f'),
            g['host_over_device_1_median'], g['host_over_device_many_median'], cell(g['host_numpy_statement'], '%.1f')))
        pr = g['pair']
        k = lambda n, c='avg_us_per_add': float(rk[(name, n)][c])
        prows.append('| %s | %.1f µs | %.1f | %.1f (%.1f) | %.1f | %.1f | %.2f (%.2f) ms | %.2f ms | %.1f %% |' % (
            shape, g['launches_ms'] * 1e3, k('k_vis_reduce'), k('k_met_ssim'), k('k_met_ssim', 'max_us_per_launch'), k('k_met_pool'), k('k_met_final'),
            pr['render_img_ms'], pr['render_img_again_ms'], pr['render_img_and_add_ms'], 100 * pr['add_share_of_pair_by_launches']))
        brows.append('%s %.1f MB read (%.1f MB of them the four inputs), %.1f MB written (the pooled levels), %.2f G f64 operations, %.1f MB of workspace, %d bytes downloaded per frame'
                     % (shape, g['bytes_read'] / 1e6, g['input_bytes'] / 1e6, g['bytes_written'] / 1e6, g['f64_operations'] / 1e9, g['workspace_bytes'] / 1e6,
                        g['download_bytes_device_route']))
        v['re_share_' + name] = '%.1f' % (100 * pr['add_share_of_pair_by_launches'])
        v['re_diff_' + name] = '%.2f' % pr['add_ms_by_difference']
        v['re_frames'], v['re_pair_iters'] = str(nf), str(pr['iters'])
    v['re_table'], v['re_pair_table'], v['re_table_bytes'] = '\n'.join(rows), '\n'.join(prows), '; '.join(brows) + '.'
    v['re_parity'] = '%.0e' % max(g['worst_mean_difference'] for g in rb['frames'].values())
    g = rb['frames']['replica']
    v['re_ssim0_replica'] = '%.0f' % float(rk[('replica', 'k_met_ssim')]['max_us_per_launch'])
    v['re_enqueue_replica'] = '%.0f' % (g['launches_ms'] * 1e3)
    w = g['windows']
    v['re_gflops'] = '%.2f' % (g['f64_operations'] * w[0] / sum(w) / 1e9)
    v['re_tflops'] = '%.0f' % (g['f64_operations'] * w[0] / sum(w) / (float(rk[('replica', 'k_met_ssim')]['max_us_per_launch']) * 1e-6) / 1e12)
    # occlusion-aware visibility against the frustum-only cull (tools/recon_bench.py --visible)
    pv = json.load(open(P('visible_bench.json')))
    q = pv['visible']
    mmm = lambda t, f='%.1f': (f + ' (' + f + ', ' + f + ')') % (t['median_ms'], t['min_ms'], t['max_ms'])
    v['pv_reps'] = str(pv['reps'])
    v['pv_faces'], v['pv_verts'] = thousands(q['faces']), thousands(q['verts'])
    v['pv_points'], v['pv_poses'] = thousands(q['points']), thousands(q['poses'])
    v['pv_visible'], v['pv_frustum'], v['pv_cull_leg'] = mmm(q['points_visible']), mmm(q['frustum_only_same_inputs'], '%.2f'), mmm(q['frustum_only_cull_leg'], '%.2f')
    qr = json.load(open(P('visible_bench_runahead.json')))['visible']
    v['pv_runahead'] = mmm(qr['points_visible'])
    v['pv_runahead_ratio'] = '%.2f' % (qr['points_visible']['median_ms'] / q['points_visible']['median_ms'])
    v['pv_runahead_again'] = '%.1f' % qr['repeat_in_the_same_run']['median_ms']
    if (qr['seen_visible'], qr['pairs_walked_share']) != (q['seen_visible'], q['pairs_walked_share']):
        v['pv_runahead'] += ' (MASKS DIFFER)'
    v['pv_never'] = thousands(q['points'] - q['seen_visible'])
    v['pv_ratio_same'], v['pv_ratio_leg'] = '%.1f' % q['visible_over_frustum_same_inputs'], '%.1f' % q['visible_over_frustum_cull_leg']
    v['pv_seen_visible'], v['pv_seen_frustum'] = thousands(q['seen_visible']), thousands(q['seen_frustum'])
    v['pv_in_frustum_share'] = '%.2f' % (100 * q['pairs_in_frustum_share'])
    v['pv_walked_share'] = '%.3f' % (100 * q['pairs_walked_share'])
    v['pv_walks_per_point'] = '%.1f' % q['walks_per_point']
    v['pv_mrays'] = '%.0f' % (q['pairs_walked_share'] * q['pairs'] / (q['points_visible']['median_ms'] * 1e-3) / 1e6)
    v['pv_same'] = 'equal' if q['pose_by_pose_equals_one_launch'] and q['visible_not_in_frustum'] == 0 else 'NOT equal'
    u = q['unseen_points']
    v['pv_unseen_ms'] = '%.1f (%.1f)' % (u['median_ms'], u['min_ms'])
    v['pv_unseen_samples'], v['pv_unseen_n'] = thousands(u['samples']), thousands(u['unseen'])
    # ---- parity / gradient stats
    t = open(P('r06_parity_stats.txt')).read()
    m = re.search(r'tol 0\.0001: (\d+) tensors, worst (\S+) of the limit', t)
    v['parity_n'], v['parity_worst'] = m.group(1), m.group(2)
    t = open(P('r06_grad_stats.txt')).read()
    tight = re.findall(r'tight, \S+: (\d+) tensors, worst element (\S+) x scale', t)
    v['grad_tight_n'] = str(sum(int(a) for a, _ in tight)); v['grad_tight_worst'] = '%.1e' % max(float(b) for _, b in tight)
    v['grad_loose_worst'] = '%.1e' % max(float(b) for b in re.findall(r'loose, \S+: \d+ parameter tensors, worst element (\S+) x scale', t))
    t = open(P('r09_grad_stats_sample_range.txt')).read()                    # the sample-count sweep (S = 1..256), rays leaving the bound, the fused path at S = 129
    tight = re.findall(r'tight, \S+: (\d+) tensors, worst element (\S+) x scale', t)
    v['grad_range_n'] = str(sum(int(a) for a, _ in tight)); v['grad_range_worst'] = '%.1e' % max(float(b) for _, b in tight)
    # ---- forward kernels of the frame
    h = stats(P('r06_kernel_stats_headline.csv'))
    for name in ('k_forward_head', 'k_sample', 'k_tsdf', 'k_decode_lc16', 'k_decode_high_g', 'k_attention_g', 'k_fallback_points', 'k_composite'):
        r = next((r for k, r in h.items() if name + '(' in k or name + '<' in k), None)
        if r:
            v[name] = '%.0f' % float(r['avg_us']) if float(r['avg_us']) >= 20 else '%.1f' % float(r['avg_us'])
    # ---- the fused iteration
    tr = stats(P('r06_kernel_stats_train.csv'))
    iters = int(next(r for k, r in tr.items() if 'k_mapper_loss' in k)['calls'])
    per = lambda *names: sum(float(r['total_ms']) * 1e3 / iters for k, r in tr.items() if any(n in k for n in names))
    zero = per('k_zero_multi')
    head = per('k_backward_head', 'k_max_reduce')
    v['train_head'] = '%.0f' % (per('k_prefilter_mask', 'k_pack_multi', 'k_forward_head', 'k_sample', 'k_tsdf(') + (zero if head else zero / 2))
    v['k_decode_lc16_train'] = '%.0f' % per('k_decode_lc16_train')
    v['train_inband_fwd'] = '%.0f' % per('k_decode_h<64', 'k_attention_h<1')
    v['train_mid'] = '%.0f' % per('k_fallback_points', 'k_composite(', 'k_mapper_loss')
    v['train_bwd_head'] = '%.0f' % (head if head else per('k_composite_bwd', 'k_bin_keys') + zero / 2)
    v['train_sort'] = '%.0f' % per('k_rs_')
    v['train_att_bwd'] = '%.0f' % per('k_attention_bwd_h', 'k_outer_h', 'k_reduce_partials_scaled')
    v['train_hl_bwd'] = '%.0f' % per('k_decode_bwd_h<')
    v['k_decode_bwd_roles'] = '%.0f' % per('k_decode_bwd_roles')
    v['k_reduce_roles'] = '%.0f' % per('k_reduce_partials_roles')
    v['k_scatter_sorted'] = '%.0f' % per('k_scatter_sorted')
    v['train_adam'] = '%.0f' % per('k_masked_adam_multi', 'k_adam_cl_multi', 'k_adam_step')
    v['n_launches'] = '%.0f' % sum(int(r['calls']) / iters for k, r in tr.items() if (k.startswith('k_') or k.startswith('void k_')) and int(r['calls']) >= iters)
    # ---- bench line
    b = json.loads(open(P('r06_bench_f16x3.json')).read().strip().split('\n')[-1])
    v['headline_value'] = '%.1f' % (b['value'] / 1e6); v['headline_ms'] = '%.2f' % b['ms_per_step']
    cfg = b['config']
    v['value_f32'] = '%.1f' % (cfg['exact_f32_value'] / 1e6)
    v['x20_value'] = '%.1f' % (cfg['value_at_x20_grids'] / 1e6)
    v['x20_parity'] = 'max-rel depth %.1e / colour %.1e' % (cfg['parity_max_rel_depth_at_x20'], cfg['parity_max_rel_color_at_x20'])
    lim = b['roofline']['limiter']
    v['loop_mfma'] = str(lim['per_tile_budget']['mfma_instructions']); v['loop_valu'] = '{:,}'.format(lim['per_tile_budget']['valu_instructions']).replace(',', ' ')
    v['limiter_cycles'] = '{:,.0f}'.format(lim['simd_cycles_per_tile']).replace(',', ' ')
    v['limiter_ceiling'] = '{:,.0f}'.format(lim['per_tile_budget']['mfma_pipe_cycles'] + 2.2 * lim['per_tile_budget']['valu_instructions']).replace(',', ' ')
    v['limiter_frac'] = '%.2f' % lim['frac_of_that_ceiling']; v['limiter_cpi'] = '%.2f' % lim['valu_issue_cycles_per_instruction']
    sm = cfg['shard_model']
    v['k8_shard_ms'] = '%.3f' % sm['k8']['ms_slowest_shard']; v['k8_ideal_ms'] = '%.3f' % (b['ms_per_step'] / 8)
    v['k8_bound_incl'] = '%.2f' % sm['k8']['speedup_bound_incl_gather']
    ro = b['roofline']
    v['avg_launch_ms'] = '%.2f' % ro['avg_launch_ms']
    v['roofline_achieved'] = '%.0f' % ro['achieved']; v['roofline_frac'] = '%.3f' % ro['frac']; v['roofline_exec_frac'] = '%.3f' % ro['frac_executed']
    pmc = ro['limiter'].get('pmc', {})
    v['mfma_busy'] = '%.3f' % pmc['mfma_busy_frac'] if 'mfma_busy_frac' in pmc else '@@mfma_busy@@'
    v['clock'] = '%.2f' % pmc['clock_ghz'] if 'clock_ghz' in pmc else '@@clock@@'
    v['traffic_bps'] = '%.1f' % (ro['traffic'] / ro['points_per_launch']) if ro.get('traffic') else '@@traffic_bps@@'
    v['tsdf_gbps'] = '%.0f' % b['roofline_tsdf']['achieved']; v['tsdf_frac'] = '%.2f' % b['roofline_tsdf']['frac']
    v['cpu_value'] = '%.0f' % b['cpu_baseline']['value']; v['cpu_cores'] = str(b['cpu_baseline']['cores'])
    rn = b.get('replica_native_frame') or b['config'].get('replica_native_frame')
    v['replica_ms'] = '%.2f' % rn['ms_per_frame']; v['replica_value'] = '%.1f' % (rn['rays_per_s'] / 1e6)
    tb = b['tracker_iteration']['by_batch']
    v['tracker_200'] = '%.3f' % tb['200']['ms_per_iteration']; v['tracker_1000'] = '%.3f' % tb['1000']['ms_per_iteration']
    c1 = b['config1']
    v['config1'] = '%.3f ms forward (%.1f M rays/s), %.2f ms forward + loss + backward through autograd' % (c1['forward']['ms'], c1['forward']['value'] / 1e6, c1['forward_backward']['ms'])
    v['config3_ms'] = '%.3f' % b['config3']['ms_per_iteration']
    v['torch_speedup'] = '%.0f' % b['torch_gpu_baseline']['speedup']
    v['shard_bound'] = '%.2f' % b['config']['shard_model']['k8']['speedup_bound']
    c5 = b['config5']; rr = c5['random_ray_order']
    v['c5_given_gbps'] = '%.0f' % rr['as_given']['tsdf_algorithmic_gbps']; v['c5_sorted_gbps'] = '%.0f' % rr['sorted']['tsdf_algorithmic_gbps']
    fb = rr['as_given'].get('tsdf_counter_bytes_per_sample')
    v['c5_fetch_b'] = '%.0f' % fb if fb else '@@c5_fetch_b@@'
    v['c5_given_ms'] = '%.2f' % rr['as_given']['ms_per_batch']; v['c5_sorted_ms'] = '%.2f' % rr['sorted']['ms_per_batch']
    v['c5_pixel_value'] = '%.1f' % (c5['value'] / 1e6)
    # ---- training
    t = open(P('r06_fused_iteration.txt')).read()
    avg = lambda xs: sum(xs) / len(xs)
    v['iter_5000'] = '%.3f' % avg([float(x) for x in re.findall(r'fused iteration, graph replay, 5000 x 64: ms per iteration (\S+)', t)])
    v['iter_5000_one_stream'] = '%.3f' % avg([float(x) for x in re.findall(r'one stream \(ADFP_SIDE_LANE=0\), graph replay, 5000 x 64: ms per iteration (\S+)', t)])
    v['iter_1000'] = '%.3f' % avg([float(x) for x in re.findall(r'1000 x 48: ms per iteration (\S+)', t)])
    for line in open(P('r06_bench_train.json')):
        if line.strip():
            r = json.loads(line)
            if r['rays'] == 5000 and r['samples_per_ray'] == 64:
                v['unchanged_5000'] = '%.2f' % r['ms_per_iter']; v['torch_floor'] = '%.2f' % r['ms_per_iter_torch_floor']
    lines = [json.loads(l) for l in open(P('r06_mapping_loop.json')) if l.strip()]
    v['loop_fused'] = '%.3f' % next(l for l in lines if l['fused'])['ms_per_iteration']
    t = open(P('r06_ab_train_forward.txt')).read()
    f = lambda pat: '%.3f' % avg([float(x) for x in re.findall(pat, t)])
    v['fwd_intree'] = f(r': (\S+) ms per call \(in-tree\)'); v['fwd_nox'] = f(r': (\S+) ms per call \(\S*NOX\.so\)')
    v['fwd_noc'] = f(r': (\S+) ms per call \(\S*NOC\.so\)')
    for row in csv.reader(l for l in open(P('r06_pmc_hbm_train.csv')) if not l.startswith('#')):
        if row and 'k_decode_lc16_train' in row[0]:
            v['lc16_train_write_B'] = '%.0f' % float(row[4]); v['lc16_train_write_MB'] = '%.0f' % (float(row[2]) / 1000.0)
    # ---- host A/B (tools/host_ab.sh): the summary lines at the end of the file
    hp = P('r06_host_ab.txt')
    if os.path.exists(hp):
        rows = re.findall(r'(round \d) (render_batch_ray \(forward\)|loss\.backward\(\))\s+host cost min\s+([\d.]+) us\s+floor min\s+([\d.]+) us\s+our share\s+([\d.]+) us', open(hp).read())
        d = {(a, sec): (float(h), float(f), float(o)) for a, sec, h, f, o in rows}
        if len(d) == 4:
            f5, f6 = d[('round 5', 'render_batch_ray (forward)')], d[('round 6', 'render_batch_ray (forward)')]
            b5, b6 = d[('round 5', 'loss.backward()')], d[('round 6', 'loss.backward()')]
            v['host_ab'] = ('`render_batch_ray` forward %.0f → %.0f µs of host time (its share above the allocation-only floor %.0f → %.0f), `loss.backward()` %.0f → %.0f (share %.0f → %.0f)'
                            % (f5[0], f6[0], f5[2], f6[2], b5[0], b6[0], b5[2], b6[2]))
    # ---- the TSDF raycast (tools/tsdfcast_bench.py)
    Q = lambda n: os.path.join(os.path.dirname(hp), n)          # (`d` is the host A/B table by now)
    tp = Q('tsdfcast_bench.json')
    if os.path.exists(tp):
        tc = json.load(open(tp))
        cell3 = lambda s, f='%.2f': (f + ' (' + f + ', ' + f + ')') % (s['median_ms'], s['min_ms'], s['max_ms'])
        rows, vols, bitmaps, worst, one_sided, samples = [], [], [], 0.0, 0, []
        for name, sc in tc['scenes'].items():
            X, Y, Z = sc['volume']
            vols.append('%s: %d × %d × %d voxels (%.2f GB), %s of %s bricks set, bitmap %.0f KB, built in %s ms.' % (
                name, X, Y, Z, sc['volume_bytes'] / 1e9, thousands(sc['bricks_set']), thousands(sc['bricks']), sc['bitmap_bytes'] / 1e3,
                cell3(sc['bricks_build'], '%.3f')))
            bitmaps.append('%.0f KB for %s' % (sc['bitmap_bytes'] / 1e3, name))
            for fname, fr in sc['frames'].items():
                at = fr.get('against_torch', {})
                worst = max(worst, at.get('max_abs_diff_m', 0.0)); one_sided = max(one_sided, at.get('one_sided_pixels', 0))
                samples.append(fr['lookups_per_ray_noskip'])
                rows.append('| %s, %d × %d | %s | %s | %s | %s | %.2f× | %s | %.1f %% of %.0f per ray | %.1f %% |' % (
                    name, fr['frame'][0], fr['frame'][1], cell3(fr['skip'], '%.3f'), cell3(fr['noskip'], '%.3f'),
                    cell3(fr['torch'], '%.0f') if 'torch' in fr else 'not measured', cell3(fr['render']), fr['noskip_over_skip'],
                    ('%.0f×' % fr['torch_over_skip']) if 'torch' in fr else 'not measured', 100 * fr['share_looked_up'], fr['lookups_per_ray_noskip'],
                    100 * fr['guide_share_of_novel_view']))
        v['tc_table'] = '\n'.join(rows); v['tc_volumes'] = '  '.join(vols); v['tc_bitmaps'] = 'It is ' + ', '.join(bitmaps)
        v['tc_reps'] = str(tc['reps']); v['tc_samples'] = '%.0f – %.0f' % (min(samples), max(samples))
        v['tc_parity'] = 'largest difference where both report a hit %.1e m, at most %d pixels of a frame hit on one side only' % (worst, one_sided)
    else:                                            # no run of tools/tsdfcast_bench.py is in the collection
        v['tc_table'] = '| not measured | | | | | | | | |'
        v['tc_volumes'] = 'No run of `tools/tsdfcast_bench.py` is in `profiles/`: none of these times has been measured.'
        v['tc_bitmaps'] = 'It is 49 KB for room0 and 93 KB for office0 (one bit per 8³ voxels of 758 × 574 × 451 and 738 × 779 × 656)'
        v['tc_reps'] = '5'; v['tc_samples'] = 'about 1 300'; v['tc_parity'] = 'not measured'
    # the whole run: where a frame's time goes (tools/run_bench.py)
    if os.path.exists(rb_path):
        rb = json.load(open(rb_path))
        a, n, o = rb['decode_ahead'], rb['no_decode_ahead'], rb['online_prior']
        rows = ['| | decode-ahead | no decode-ahead | `--prior online` |', '|---|---|---|---|']
        for label, key, fmt in (('tracked frame: fetch + tracking, ms', 'track_frame_ms', '%.2f'), ('… of which tracking (10 replays, the pose download)', 'track_only_ms', '%.2f'),
                                ('… of which fetch (wait for the decode, upload, ingest)', 'fetch_ms', '%.2f'),
                                ('tracked frame right after a mapped one (graphs re-captured), ms', 'track_frame_after_map_ms', '%.2f'),
                                ('mapped frame, ordinary (60 iterations, selection, masks), ms', 'map_frame_ms', '%.2f'),
                                ('mapped frame 0 (1500 iterations, captures), ms', 'map_first_frame_ms', '%.0f'),
                                ('last frame (colour refinement, checkpoint, 128³ mesh), ms', 'map_last_frame_ms', '%.0f'),
                                ('host decode of one frame (JPEG + PNG), ms', 'decode_ms', '%.2f'), ('… the loop waited for it, ms', 'decode_wait_ms', '%.2f'),
                                ('GPU-idle share of a tracked frame (lower bound)', 'gpu_idle_share', '%.2f'), ('whole run of %d frames, s' % a['frames'], 'wall_s', '%.2f')):
            rows.append('| %s | %s |' % (label, ' | '.join((fmt % r[key]) if r.get(key) is not None else '' for r in (a, n, o))))
        relay = ('%.2f ms' % o['relay_corner_blocks_ms']) if o.get('relay_corner_blocks_ms') is not None else 'not taken (no corner-block copy)'
        v['rb_numbers'] = ('Measured on one MI355X (`profiles/run_bench.json`; volume %s voxels, medians over the frames of one run each):\n\n' % ' × '.join(str(x) for x in rb['volume'])
                           + '\n'.join(rows) + '\n\n'
                           + 'The tracked frame\'s %d iterations replayed back to back take %.2f ms between two events (%.2f ms each; `README.md` quotes 0.15 ms), '
                             'so the GPU is idle for at least %.0f %% of a tracked frame with decode-ahead and %.0f %% without.  '
                             'The decode (%.1f ms) is the largest single item of a tracked frame, as expected, but it is not several times the rest: decode-ahead hides %.1f of '
                             'its %.1f ms and takes the tracked frame from %.2f to %.2f ms.  '
                             'Online prior, per mapped frame: one integrate %.2f ms and one full re-lay of the %.1f GB corner-block copy %s, each timed alone with synchronises; '
                             'the mapped frame is %.2f ms longer than with the fused prior (%.2f against %.2f ms), %.0f %% of it -- not material beside 60 iterations, '
                             'so the incremental re-lay is not the next thing to build.'
                           % (rb['iterations']['tracking'][0], a['track_gpu_ms'], a['track_gpu_ms'] / rb['iterations']['tracking'][0], 100 * a['gpu_idle_share'], 100 * n['gpu_idle_share'],
                              a['decode_ms'], n['decode_wait_ms'] - a['decode_wait_ms'], n['decode_wait_ms'], n['track_frame_ms'], a['track_frame_ms'],
                              o['integrate_ms'], o['corner_block_bytes'] / 1e9, relay, o['map_frame_minus_fused_prior_ms'], o['map_frame_ms'], a['map_frame_ms'],
                              100 * o['map_frame_minus_fused_prior_ms'] / o['map_frame_ms']))
    else:
        v['rb_numbers'] = 'No run of `tools/run_bench.py` is in `profiles/`: not measured.'
    # bundle adjustment beside the plain Mapper iteration (tools/ba_bench.py)
    if os.path.exists(ba_path):
        ba = json.load(open(ba_path))
        rows = ['| stage | BA off, ms per iteration | BA on, ms per iteration | on / off |', '|---|---|---|---|']
        for st in ('low', 'high', 'color'):
            r = ba['stages'][st]
            rows.append('| %s | %.3f (blocks %.3f – %.3f) | %.3f (blocks %.3f – %.3f) | %.2f× |' % (
                st, r['ms_per_iter_ba_off'], min(r['ba_off_blocks_ms']), max(r['ba_off_blocks_ms']),
                r['ms_per_iter_ba_on'], min(r['ba_on_blocks_ms']), max(r['ba_on_blocks_ms']), r['ratio_on_over_off']))
        v['ba_numbers'] = ('Measured on one MI355X (`profiles/ba_bench.json`): the %s iteration of %d rays × %d samples over a %d-frame window, sampling '
                           'included, graph replay, the two modes alternating in blocks of %d iterations (%d blocks each, medians; host clock around a '
                           'device synchronise):\n\n' % (ba['scene'], ba['rays'], ba['samples_per_ray'], ba['frames'], ba['iters_per_block'], ba['rounds'])
                           + '\n'.join(rows) + '\n\n'
                           + 'The head alone takes %.1f µs and the tail alone %.1f µs per launch, launched back to back between two events, so nearly all of the '
                             'difference is the backward itself: asked for ray cotangents together with grid and weight gradients it runs the exact f32 '
                             'kernels for every network (`Engine.ht_nets`); it has not been traced kernel by kernel for this case.  '
                             'No threshold is set: what the ray-gradient path costs beside the grid gradients is the ratio above.  '
                             'Beside the BA-off figure of stage color (%.3f ms: ten poses, a fresh draw and one sampling launch per iteration) stands '
                             '`bench_train.py`\'s fused graph-replayed iteration of the collection before this feature (`profiles/r06_bench_train.json`: '
                             'one pose, a fixed batch of 5 000 rays × 64 samples, stage color): %.3f ms.'
                           % (ba['head_us_per_call_back_to_back'], ba['tail_us_per_call_back_to_back'], ba['stages']['color']['ms_per_iter_ba_off'],
                              bench_train_5000x64))
    else:
        v['ba_numbers'] = 'No run of `tools/ba_bench.py` is in `profiles/`: not measured.'
    # mesh simplification: the device call beside the numpy statement (tools/simplify_bench.py)
    sb_path = Q('simplify_bench.json')
    if os.path.exists(sb_path):
        sb = json.load(open(sb_path))
        rows = ['| voxel | contraction | vertices | faces | host numpy statement, ms | device call, ms | host / device | accuracy, cm | completion, cm | within 5 cm, % |',
                '|---|---|---|---|---|---|---|---|---|---|']
        label = {'1x': '1 × spacing', '2x': '2 × spacing', '4x': '4 × spacing', 'model': '4 × the model\'s extent (one cell)'}
        for key, r in sb['cases'].items():
            name, contraction = key.rsplit('_', 1)
            met = ('%.3f | %.3f | %.2f' % (r['accuracy_cm'], r['completion_cm'], r['completion_ratio_pct'])) if r.get('accuracy_cm') is not None else '– | – | –'
            rows.append('| %s | %s | %s | %s | %s | %s | %.1f× | %s |' % (
                label[name], contraction, thousands(r['verts_out']), thousands(r['faces_out']), cell(r['host']), cell(r['device'], '%.3f'),
                r['host_over_device_median'], met))
        agree = all(r['faces_equal'] for r in sb['cases'].values())
        worst = max(r['max_position_difference'] for r in sb['cases'].values())
        floor = sb['mesh_against_itself']
        mq, ma = sb['cases']['model_quadric']['device'], sb['cases']['model_average']['device']
        v['sb_numbers'] = ('Measured on one MI355X (`profiles/simplify_bench.json`, one run of `tools/simplify_bench.py --reps %d`): the cleaned %s mesh of '
                           '%s vertices and %s faces, lattice spacing %.4f m, workspace %.1f MB.  Both sides alternate in the one run, wall clock with a device '
                           'synchronisation on both ends; milliseconds, median (min, spread = max − min).  The device call is plan + the read-back of the two totals + '
                           'emit; the host side is the tests\' numpy statement of the same rules (`tests/simplify_ref.py`), not a tuned implementation, so the ratio '
                           'says what the statement costs and nothing about open3d, which was never run.  Accuracy, completion and completion ratio are `recon.py`\'s, '
                           '%s seeded surface samples per mesh, simplified against unsimplified, no alignment:\n\n' % (
                               sb['reps'], sb['workload'].split(',')[0], thousands(sb['verts']), thousands(sb['faces']), sb['lattice_spacing'],
                               sb['workspace_bytes'] / 1e6, thousands(sb['samples']))
                           + '\n'.join(rows) + '\n\n'
                           + 'The two sides\' faces are %s in every case and their positions differ by at most %.1e m (0 = the same f32 values).  The metric has a floor: the unsimplified mesh '
                             'against itself, through the same two independent draws, measures accuracy %.3f cm, completion %.3f cm, %.2f %% -- the spacing of %s samples '
                             'over the room\'s surface -- so the rows above are read against that, not against zero.  '
                             'The degenerate call, one cell holding every vertex, returns the empty mesh after %.1f ms (average) and %.0f ms (quadric): one lane walks all %s '
                             'vertices in `k_vds_mean` and `k_msp_cells`, and in `k_msp_quadric` all %s contributions with three dependent gathers and an f64 square root and '
                             'three divisions each.' % (
                                 'equal element for element' if agree else 'NOT equal', worst, floor['accuracy_cm'], floor['completion_cm'],
                                 floor['completion_ratio_pct'], thousands(sb['samples']), ma['median_ms'], mq['median_ms'], thousands(sb['verts']),
                                 thousands(3 * sb['faces'])))
    else:
        v['sb_numbers'] = 'No run of `tools/simplify_bench.py` is in `profiles/`: not measured.'
    # mesh colours from the keyframes: the device call beside the numpy statement (tools/color_mesh_bench.py)
    cm_path = Q('color_mesh_bench.json')
    if os.path.exists(cm_path):
        cm = json.load(open(cm_path))
        cases = cm['cases']
        first = next(iter(cases.values()))
        rows = ['| keyframes | blend | device call, ms | numpy statement on %s vertices, s | covered vertices | pairs in frame / all pairs | contributing pairs '
                '| colour difference, byte steps |' % thousands(cm['host_vertices']), '|---|---|---|---|---|---|---|---|']
        for name, r in cases.items():
            K, blend = name.split('_')
            rows.append('| %s | %s | %.3f (%.3f) | %.3f | %.1f %% | %s / %s | %s | %.2f |' % (
                K, blend, r['device']['median_ms'], r['device']['min_ms'], r['host_s'], 100 * r['covered_share'], thousands(r['pairs_in_frame']),
                thousands(r['pairs']), thousands(r['pairs_contributing']), r['image_difference_keyframe_projection']))
        agree = all(r['count_equal_share'] == 1.0 and r['best_equal_share'] == 1.0 for r in cases.values())
        worst = max(r['max_colour_difference_where_counts_agree'] for r in cases.values())
        last = list(cases.values())[-2]
        frame = [r['pairs_in_frame'] / r['pairs'] for r in cases.values()]
        contrib = [r['pairs_contributing'] / r['pairs_in_frame'] for r in cases.values()]
        blends = max(abs(cases[a]['image_difference_keyframe_projection'] - cases[b]['image_difference_keyframe_projection'])
                     for a, b in zip(list(cases)[0::2], list(cases)[1::2]))
        v['cm_numbers'] = (
            'Measured on one MI355X on %s (`profiles/color_mesh_bench.json`, one run of `tools/color_mesh_bench.py`): the cleaned %s mesh at 512³ '
            '(%s vertices, %s faces) against synthetic keyframes at Replica\'s frame (680 × 1200, f = 600) on `tools/mesh_bench.py`\'s many-pose path, '
            'analytic depth with its band of zero depth, a smooth analytic texture, `depth_tol` %g, `border` %d.  The device call is `mesh.project_colors` '
            '(the poses\' read-back and inversion on the host, the launch): %d calls back to back between two device synchronisations, %d such repetitions, '
            'milliseconds per call, median (min).  The host side is the tests\' numpy statement on every %dth vertex (%s), run once: not a tuned '
            'implementation, so its time says what the statement costs.  The colour difference is the mean absolute difference, in byte steps, between '
            'the mesh rendered through `render_mesh`\'s colour view (`MeshViews.render`, mode `color`) at the first %d keyframes\' poses and those '
            'keyframes\' images, over the %s pixels where the mesh is hit and the keyframe has depth; the direct point query\'s colours (the seed-initialised '
            'colour decoder\'s, which no one trained) measure %.2f there.\n\n' % (
                cm['date'], cm['workload'].split(',')[0], thousands(cm['verts']), thousands(cm['faces']), cm['depth_tol'], cm['border'], cm['calls_per_rep'],
                cm['reps'], round(cm['verts'] / cm['host_vertices']), thousands(cm['host_vertices']), first['image_difference_views'],
                thousands(first['image_difference_pixels']), first['image_difference_direct_point_query'])
            + '\n'.join(rows) +
            '\n\nOn the %s vertices that both sides computed, `count` and `best` are %s and the colours differ by at most %.1e (0 = the same f32 values) '
            'over the %d cases.  Between %.0f %% and %.0f %% of the pairs pass the frame test, and of those between %.0f %% and %.0f %% contribute: the '
            'others fall on the zero-depth band, face a keyframe whose depth at their pixel lies further away than the tolerance, or straddle a depth '
            'edge.  Which of the three dominates was not measured.  %.0f %% of the vertices stay uncovered at %s keyframes and keep the decoder\'s '
            'colour -- the level set of a seed-initialised decoder is not the room\'s walls everywhere -- so the colour difference falls with the covered '
            'share instead of reaching zero.  The two blends differ by at most %.2f byte steps here: the texture is smooth and the poses exact, so every '
            'view of a vertex shows the same colour.  No kernel trace was collected; per vertex-keyframe pair the largest weighted call costs %.1f ps, '
            'which includes the host\'s share of the call.' % (
                thousands(cm['host_vertices']), 'equal everywhere' if agree else 'NOT equal everywhere', worst, len(cases), 100 * min(frame), 100 * max(frame),
                100 * min(contrib), 100 * max(contrib), 100 * (1 - last['covered_share']), list(cases)[-2].split('_')[0], blends,
                last['device']['median_ms'] * 1e9 / last['pairs']))
    else:
        v['cm_numbers'] = 'No run of `tools/color_mesh_bench.py` is in `profiles/`: not measured.'
    # depth ICP beside the tracking it precedes (tools/icp_bench.py)
    ic_path = Q('icp_bench.json')
    if os.path.exists(ic_path):
        ic = json.load(open(ic_path))
        cell3 = lambda s, f='%.3f': (f + ' (' + f + ', ' + f + ')') % (s['median_ms'], s['min_ms'], s['max_ms'])
        rows = ['| leg | ms, median (min, max) |', '|---|---|']
        for label, key in (('raycast of the model from the guess', 'raycast'), ('normal maps of both images, one launch', 'normals'),
                           ('one step at stride 4 (with `adfp_icp_begin`)', 'step_s4'), ('one step at stride 2', 'step_s2'),
                           ('one step at stride 1', 'step_s1'), ('begin, the ten steps, end', 'steps'),
                           ('`refine` as a whole', 'refine'), ('`new_frame` and ten `TrackerIteration.step` replays of 200 pixels', 'track10')):
            rows.append('| %s | %s |' % (label, cell3(ic[key])))
        v['icp_numbers'] = ('Measured on one MI355X (`profiles/icp_bench.json`, one run of `tools/icp_bench.py --reps %d`): Replica\'s frame, %d × %d, in '
                            'the room0 box-room volume (%s voxels), a corner-facing pose inside the room, the sensor depth the raycast at the true pose, the '
                            'guess %.1f mm and %.2f° off; strides %s with %s steps.  Device events around each leg, the legs alternating within a repetition:\n\n'
                            % (ic['reps'], ic['frame'][0], ic['frame'][1], ' × '.join(str(x) for x in ic['volume']), ic['error_before_m_rad'][0] * 1e3,
                               ic['error_before_m_rad'][1] * 57.29577951308232, ', '.join(str(x) for x in ic['levels']['strides']),
                               ', '.join(str(x) for x in ic['levels']['iters']))
                            + '\n'.join(rows) + '\n\n'
                            + 'The refinement ended with status %d (0 = OK) %.2f mm and %.3f° from the true pose, on %s to %s pairs per step (%s and %s valid normals '
                              'in the sensor and the model image), smallest pivot ratio %.1e.  `refine` takes %.2f × the time of the ten tracking iterations it precedes.  '
                              'No threshold is set and no speed target: these are the first times of this path.'
                            % (ic['status'], ic['error_after_m_rad'][0] * 1e3, ic['error_after_m_rad'][1] * 57.29577951308232,
                               thousands(int(min(ic['pairs_per_step']))), thousands(int(max(ic['pairs_per_step']))), thousands(ic['valid_sensor_normals']),
                               thousands(ic['valid_model_normals']), ic['pivot_ratio_min'], ic['refine_over_track10']))
    else:
        v['icp_numbers'] = 'No run of `tools/icp_bench.py` is in `profiles/`: not measured.'
    # RGB-D ICP beside the depth ICP (tools/icp_bench.py --rgbd-json)
    rg_path = Q('rgbd_icp_bench.json')
    if os.path.exists(rg_path):
        rg = json.load(open(rg_path))
        cell3 = lambda s, f='%.3f': (f + ' (' + f + ', ' + f + ')') % (s['median_ms'], s['min_ms'], s['max_ms'])
        rows = ['| leg | ms, median (min, max) |', '|---|---|']
        for label, key in (('frame map of one frame (`adfp_rgbd_frame_map`)', 'frame_map'),
                           ('one joint step at stride 4 (with `adfp_icp_begin`)', 'joint_s4'), ('… the depth-only step beside it', 'step_s4'),
                           ('one joint step at stride 2', 'joint_s2'), ('… the depth-only step beside it', 'step_s2'),
                           ('one joint step at stride 1', 'joint_s1'), ('… the depth-only step beside it', 'step_s1'),
                           ('`promote` (the map\'s copy, the pose\'s upload)', 'promote'),
                           ('`RgbdICP.refine` as a whole (with `set_keyframe` before it)', 'rgbd_refine'), ('`DepthICP.refine` beside it', 'refine')):
            rows.append('| %s | %s |' % (label, cell3(rg[key])))
        v['rgbd_numbers'] = ('Measured on one MI355X (`profiles/rgbd_icp_bench.json`, one run of `tools/icp_bench.py --reps %d --rgbd-json`): section 5.13\'s '
                             'frame, %d × %d, the colour `tests/test_gpu_slam_run.py`\'s rule at every pixel\'s world point, the keyframe the scene seen from '
                             '%.0f mm and %.0f mrad away, `rgb_weight` %g, `rgb_tol` %g.  Device events around each leg, the legs alternating within a '
                             'repetition:\n\n'
                             % (rg['reps'], rg['frame'][0], rg['frame'][1], rg['keyframe_distance_m_rad'][0] * 1e3, rg['keyframe_distance_m_rad'][1] * 1e3,
                                rg['rgb_weight'], rg['rgb_tol'])
                             + '\n'.join(rows) + '\n\n'
                             + 'The refinement ended with status %d (0 = OK) %.2f mm and %.3f° from the true pose (the guess: %.1f mm, %.2f°), on %s to %s '
                               'geometric and %s to %s photometric pairs per step, smallest pivot ratio %.1e.  `RgbdICP.refine` takes %.2f × the time of '
                               '`DepthICP.refine`.  No threshold is set and no speed target: these are the first times of this path.'
                             % (rg['status'], rg['error_after_m_rad'][0] * 1e3, rg['error_after_m_rad'][1] * 57.29577951308232,
                                rg['error_before_m_rad'][0] * 1e3, rg['error_before_m_rad'][1] * 57.29577951308232,
                                thousands(int(min(rg['pairs_per_step']))), thousands(int(max(rg['pairs_per_step']))),
                                thousands(int(min(rg['rgb_pairs_per_step']))), thousands(int(max(rg['rgb_pairs_per_step']))), rg['pivot_ratio_min'],
                                rg['rgbd_refine_over_refine']))
    else:
        v['rgbd_numbers'] = 'No run of `tools/icp_bench.py --rgbd-json` is in `profiles/`: the times of this path have not been measured.'
    # the depth bilateral filter alone and in front of the refinement (tools/icp_bench.py --filter-json)
    fl_path = Q('icp_filter_bench.json')
    if os.path.exists(fl_path):
        fl = json.load(open(fl_path))
        cell3 = lambda s, f='%.3f': (f + ' (' + f + ', ' + f + ')') % (s['median_ms'], s['min_ms'], s['max_ms'])
        rows = ['| leg | ms, median (min, max) |', '|---|---|']
        for label, key in (('the filter alone, %d × %d, radius 2' % tuple(fl['frame']), 'filter_r2'), ('… radius 3', 'filter_r3'),
                           ('the filter alone, %d × %d (TUM RGB-D), radius 2' % tuple(fl['tum_frame']), 'filter_tum_r2'),
                           ('… radius 3', 'filter_tum_r3'), ('clean depth: `DepthICP.refine` without the filter (the comparator)', 'refine'),
                           ('clean depth: `DepthICP(bilateral={}).refine`', 'refine_bilateral'),
                           ('noisy depth: `DepthICP.refine` without the filter', 'refine_noisy'),
                           ('noisy depth: `DepthICP(bilateral={}).refine`', 'refine_noisy_bilateral'),
                           ('noisy depth: … with `points: false`', 'refine_noisy_bilateral_raw_points')):
            rows.append('| %s | %s |' % (label, cell3(fl[key])))
        off, on, cl = fl['refine_noisy'], fl['refine_noisy_bilateral'], fl['refine_bilateral']
        deg = 57.29577951308232
        v['filter_numbers'] = ('Measured on one MI355X (`profiles/icp_filter_bench.json`, one run of `tools/icp_bench.py --reps %d --filter-json`): section '
                               '5.13\'s frame and pose, clean (the raycast at the true pose) and through `synthetic.sensor_depth`\'s default model '
                               '(depths %.2f – %.2f m), and the same scene at TUM RGB-D\'s frame; the filter\'s defaults but for the radius.  Device events '
                               'around each leg, the legs alternating within a repetition; the clean refinement without the filter is the path before '
                               'this section, timed in the same run:\n\n' % (fl['reps'], fl['sensor_depth_range_m'][0], fl['sensor_depth_range_m'][1])
                               + '\n'.join(rows) + '\n\n'
                               + 'On clean depth both refinements go through all ten steps: the filter\'s launch at radius 2 is %.1f %% of the filtered '
                                 '`refine`, which takes %.2f × the unfiltered one (%+.3f ms) and ends with status %d (0 = OK) %.2f mm and %.3f° from the true '
                                 'pose against %.2f mm and %.3f° unfiltered -- the clean-depth cost again.  On the noisy frame the unfiltered refinement '
                                 'ended with status %d on %s pairs in its first step (a refinement that fails does nothing in its remaining steps, hence '
                                 'its short time) and returned the guess, %.1f mm and %.2f° off; the filtered one ended with status %d on %s to %s pairs '
                                 'per step, %.2f mm and %.3f° from the true pose, and with `points: false` %.2f mm and %.3f°.  No threshold is set and no '
                                 'speed target: these are the first times of this path.'
                               % (100 * fl['filter_share_of_refine'], fl['refine_bilateral_over_refine'], fl['refine_bilateral_minus_refine_ms'],
                                  cl['status'], cl['error_after_m_rad'][0] * 1e3, cl['error_after_m_rad'][1] * deg,
                                  fl['refine']['error_after_m_rad'][0] * 1e3, fl['refine']['error_after_m_rad'][1] * deg,
                                  off['status'], thousands(int(off['pairs_per_step'][0])), fl['error_before_m_rad'][0] * 1e3, fl['error_before_m_rad'][1] * deg,
                                  on['status'], thousands(int(min(on['pairs_per_step']))), thousands(int(max(on['pairs_per_step']))),
                                  on['error_after_m_rad'][0] * 1e3, on['error_after_m_rad'][1] * deg,
                                  fl['refine_noisy_bilateral_raw_points']['error_after_m_rad'][0] * 1e3,
                                  fl['refine_noisy_bilateral_raw_points']['error_after_m_rad'][1] * deg))
    else:
        v['filter_numbers'] = 'No run of `tools/icp_bench.py --filter-json` is in `profiles/`: the times of this path have not been measured.'
    s = open(template).read()
    out = re.sub(r'@@(\w+)@@', lambda m: v.get(m.group(1), m.group(0)), s)
    sys.stdout.write(out)
    left = sorted(set(re.findall(r'@@(\w+)@@', out)))
    if left:
        sys.stderr.write('unfilled: ' + ', '.join(left) + '\n')


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
