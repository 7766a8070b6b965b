"""What the CPU tests of the accumulators behind the z update (per-site intervals, convergence diagnostics, held-out scoring)
read off the text of occ_gibbs.hip: occ_get_stats counts no launches per kernel, so "the kernel is launched only while a
switch is on, and a run with the switch never touched enqueues what it enqueued before" is pinned on launch_kind and on the
one place that writes the word which guards the launch."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'occuspytial_amd', 'csrc')

# feature -> (what is launched just before it behind the z update, its run-time struct in occ_sampler)
BEHIND_Z = {'hist': (r'sp_launch\(s->spatial\.args', r'struct Hist : AccumRun \{'),
            'conv': (r'hist_launch\(s->hist\.args', r'struct Conv : AccumRun \{'),
            'holdout': (r'conv_launch\(s->conv\.args', r'struct Holdout : AccumRun \{')}


def unit_text(name):
    return open(os.path.join(CSRC, name)).read()


def assert_launched_only_while_on(feature):
    """The one call of <feature>_launch stands behind `if (s-><feature>.any)`, directly after the launch before it in the order
    sp -> hist -> conv -> holdout; the word is Switches::any, which starts at 0 and is written in one place of the whole file,
    switch_set, which the spatial residual check and all three accumulators reach; occ_profile clears it for its scope."""
    src = unit_text('occ_gibbs.hip')
    before, struct = BEHIND_Z[feature]
    f = feature
    assert len(re.findall(r'\b%s_launch\(' % f, src)) == 1
    assert re.search(before + r'[^\n]*\n\s*if \(s->%s\.any\)[^\n]*\n\s*%s_launch\(s->%s\.args, s->ctx\.sc, c\.C, e, st\);' % (f, f, f), src)
    # the word: one declaration, default 0u, inherited by the feature's struct
    assert len(re.findall(r'uint32_t any = 0u;', src)) == 2        # Switches::any and switch_set's local
    assert re.search(r'struct Switches \{\s*uint32_t any = 0u;', src)
    assert re.search(r'struct AccumRun : Switches \{', src) and re.search(struct, src)
    assert re.search(r'struct Spatial : Switches \{', src)
    # one assignment to a member `any` in the whole file, in switch_set ...
    assert re.findall(r'(?:\.|->)any = ([^;]+);', src) == ['any']
    body = re.search(r'static int switch_set\(occ_sampler \*s, occ_sampler::Switches &sw, int chain, bool on\)\n\{(.*?)\n\}\n', src, re.S).group(1)
    assert 'if (any != sw.any) destroy_graph(s);\n    sw.any = any;' in body
    # ... which all four features reach: the spatial check by itself, the accumulators through set_accum_state and accum()
    assert len(re.findall(r'\bswitch_set\(', src)) == 3
    assert re.search(r'static int moran_switch\(.*?\n    return switch_set\(s, sp, chain, on\);\n\}', src, re.S)
    assert re.search(r'static int set_accum_state\(.*?occ_sampler::AccumRun &r = s->accum\(kind\);.*?\n    return switch_set\(s, r, chain, val != 0\);\n\}', src, re.S)
    assert re.search(r'AccumRun &accum\(int kind\) \{ return kind == ACC_HIST \? \(AccumRun &\)hist : kind == ACC_CONV \? \(AccumRun &\)conv : '
                     r'\(AccumRun &\)holdout; \}', src)
    # nothing else takes its address but occ_profile's clears
    assert sorted(re.findall(r'&s->(\w+)\.any\b', src)) == ['conv', 'hist', 'holdout', 'spatial']
    assert re.search(r'Scoped<uint32_t> no_%s\(&s->%s\.any, 0u\);' % (f, f), src)
