// Kernel-level C-ABI entry points (single layers): the per-layer parity tests (tests/test_gpu_layers.py), the planner-coverage test
// (tests/test_cpu_forms.py), the glue-kernel and whole-network pack-launch tests (tests/test_gpu_aux.py; ocl_test_head, which needs the
// engine's head functions, lives in net.hip) and micro-benchmarks.  They plan, finalize, pack and launch through the engine's own
// functions; no kernel lives here.
#include "conv.h"
#include <string.h>
#include <algorithm>
#include <vector>

using namespace ocl;

namespace ocl {

ConvShape test_conv_shape(const ocl_test_conv_desc& d) {
    ConvShape s;
    memset(&s, 0, sizeof(s));
    s.Cin = d.cin; s.CinT = d.cin == 3 ? 4 : d.cin; s.Cout = d.cout; s.k = d.k; s.stride = d.stride;
    s.Hin = d.hin; s.Win = d.win;
    const int pad = d.k == 3 ? 1 : 0;
    s.Ho = (d.hin + 2 * pad - d.k) / d.stride + 1;
    s.Wo = (d.win + 2 * pad - d.k) / d.stride + 1;
    s.CoutP = pack_width(d.cout);
    s.CiP = d.cin == 3 ? 0 : pack_width(d.cin);
    return s;
}

// the geometries of a layer's launches, chosen as net.hip's make_plan_set chooses them
static int test_conv_geoms(const ocl_test_conv_desc& d, std::vector<ConvGeomDesc>* out) {
    OCL_REQUIRE(d.n > 0 && d.groups > 0 && (d.k == 1 || d.k == 3) && (d.stride == 1 || d.stride == 2) && d.hin > 0 && d.win > 0 &&
                    (d.cin == 3 || d.cin % 4 == 0) && d.cout % 4 == 0 && (d.dir == 0 || d.dir == 1),
                "test_conv: bad layer description");
    const ConvShape c = test_conv_shape(d);
    out->clear();
    if (d.dir == 0) {
        ConvGeomDesc g;
        geom_fwd(c, d.n, d.groups, &g);
        g.xf = d.xf;
        out->push_back(g);
    } else {
        OCL_REQUIRE(d.cin != 3, "test_conv: the stem has no data gradient");
        geom_dgrad(c, d.n, out, d.merge != 0, d.bnb ? d.groups : 1);
        if (d.bnb && out->size() == 1) (*out)[0].bnb = 1;
        if (out->size() == 1 && (*out)[0].ncls > 1) {
            ConvPlan p;
            if (plan_conv((*out)[0], &p) != OCL_OK) geom_dgrad(c, d.n, out, false);
        }
    }
    for (auto& g : *out) {
        g.force_MT = d.force_mt; g.force_NT = d.force_nt; g.force_pipe = d.force_pipe;
        g.force_q4 = d.force_q4; g.force_cs = d.force_cs; g.force_cw = d.force_cw;
    }
    return OCL_OK;
}

void test_conv_form(const ConvPlan& p, ocl_test_conv_form* f) {
    memset(f, 0, sizeof(*f));
    const ConvArgs& a = p.a;
    f->family = p.cw == 2 ? 4 : p.cw ? 3 : p.cs ? 2 : p.q4 ? 1 : 0;
    f->mt = p.MT; f->nt = p.NT; f->q4 = p.q4; f->pipe = a.pipe; f->wres = a.wres; f->ncls = a.cls_pack & 15;
    // the prefetch depth of the instantiation launch_conv picks (conv_t: the engine's convt_plan_pf; conv_q: the plan's staging table)
    f->pf = p.q4 ? (a.off_loc - a.off_pu) / (3 * 256) : (p.cs || p.cw) ? 0 : convt_plan_pf(p);
    f->bnb_room = a.bnb_lds >= 0 ? 1 : 0;
    f->grid_x = p.grid_x; f->grid_y = p.grid_y;
}

void test_wgrad_form(const WgradPlan& p, ocl_test_wgrad_form* f) {
    memset(f, 0, sizeof(*f));
    f->mtw = p.MTW; f->ntw = p.NTW; f->q_rgw = p.q_rgw;
    f->pf = wgrad_plan_pf(p);
    f->multi = wgrad_multi_variant(p);
    f->s = p.a.S; f->grid_x = p.grid_x; f->grid_y = p.grid_y;
}

}  // namespace ocl

namespace {

// device scratch of one hook call, freed (after the stream has drained) when the call returns
struct Scratch {
    std::vector<void*> bufs;
    hipStream_t s = nullptr;
    void* take(size_t bytes, int fill) {
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(bytes, 256)) != hipSuccess) return nullptr;
        bufs.push_back(p);
        if (hipMemsetAsync(p, fill, std::max<size_t>(bytes, 256), s) != hipSuccess) return nullptr;
        return p;
    }
    ~Scratch() {
        (void)hipStreamSynchronize(s);
        for (void* p : bufs) (void)hipFree(p);
    }
};

int wgrad_plan_of(const ocl_test_wgrad_desc& d, WgradPlan* p) {
    OCL_REQUIRE(d.n > 0 && (d.k == 1 || d.k == 3) && (d.stride == 1 || d.stride == 2) && (d.cin == 3 || d.cin % 4 == 0) && d.cout % 4 == 0,
                "test_wgrad: bad layer description");
    ocl_test_conv_desc cd;
    memset(&cd, 0, sizeof(cd));
    cd.cin = d.cin; cd.cout = d.cout; cd.k = d.k; cd.stride = d.stride; cd.hin = d.hin; cd.win = d.win;
    const ConvShape c = test_conv_shape(cd);
    return plan_wgrad(d.n, c.Hin, c.Win, c.CinT, c.Ho, c.Wo, c.Cout, c.k, c.stride, p, d.xf_groups, d.wg_target);
}

}  // namespace

extern "C" {

int ocl_bn_bwd_nhwc(const float* dz, const float* zmask, const float* y, const float* mean, const float* invstd, const float* gamma,
                    int64_t m_per_group, int groups, int c, float* dy, float* dgamma, float* dbeta, int accumulate, double* scratch,
                    void* stream) {
    OCL_REQUIRE(dz && y && mean && invstd && gamma && dy && dgamma && dbeta && scratch, "bn_bwd: null pointer");
    OCL_REQUIRE(m_per_group > 0 && groups > 0 && c > 0 && c % 4 == 0 && c <= 1024, "bn_bwd: bad sizes");
    hipStream_t s = (hipStream_t)stream;
    OCL_HIP(hipMemsetAsync(scratch, 0, (size_t)groups * 2 * c * sizeof(StatCell), s));   // (one 16-byte accumulator cell per sum)
    BnBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.dz = dz; a.z = zmask; a.m_per_group = m_per_group; a.G = groups; a.C = c; a.nsets = 1;
    a.y[0] = y; a.mean[0] = mean; a.invstd[0] = invstd; a.gamma[0] = gamma; a.dy[0] = dy; a.dgamma[0] = dgamma; a.dbeta[0] = dbeta;
    a.sums = (StatCell*)scratch;
    a.accumulate = accumulate;
    return launch_bn_bwd(a, s);
}

int ocl_test_conv_plan(const ocl_test_conv_desc* desc, ocl_test_conv_form* forms, int cap) {
    OCL_REQUIRE(desc, "test_conv_plan: null pointer");
    std::vector<ConvGeomDesc> gs;
    int rc = test_conv_geoms(*desc, &gs);
    if (rc != OCL_OK) return rc;
    for (size_t i = 0; i < gs.size(); ++i) {
        ConvPlan p;
        if ((rc = plan_conv(gs[i], &p)) != OCL_OK) return rc;
        if ((int)i < cap && forms) test_conv_form(p, &forms[i]);
    }
    return (int)gs.size();
}

int ocl_test_conv(const ocl_test_conv_desc* desc, const ocl_test_conv_ops* o, ocl_test_conv_form* forms, int cap, void* stream) {
    OCL_REQUIRE(desc && o && o->in && o->w && o->out, "test_conv: null pointer");
    const ocl_test_conv_desc& d = *desc;
    OCL_REQUIRE(!(o->flags & (EPI_STATS | EPI_BNB)) || o->stats, "test_conv: EPI_STATS / EPI_BNB without cells");
    OCL_REQUIRE(!o->xf || (d.xf && d.dir == 0 && o->xf_stats && o->xf_gamma && o->xf_beta && o->xf_save_mean && o->xf_save_invstd),
                "test_conv: input transform without its reservation / operands");
    OCL_REQUIRE(!(o->flags & EPI_BNB) || (d.bnb && d.dir == 1 && o->bnb_y && o->bnb_mean && o->bnb_invstd && o->bnb_gamma && o->bnb_beta),
                "test_conv: EPI_BNB without its reservation / operands");
    int rc = conv_kernels_init();
    if (rc != OCL_OK) return rc;
    std::vector<ConvGeomDesc> gs;
    if ((rc = test_conv_geoms(d, &gs)) != OCL_OK) return rc;
    const ConvShape c = test_conv_shape(d);
    hipStream_t s = (hipStream_t)stream;
    Scratch sc;
    sc.s = s;
    // the weight pack of this direction, written by the engine's pack kernel from the OIHW tensor (padding rows stay zero)
    PackDesc pd;
    memset(&pd, 0, sizeof(pd));
    pd.w_off = 0; pd.Cout = c.Cout; pd.Cin = c.Cin; pd.ntaps = c.k * c.k; pd.CinP = c.CinT; pd.CoutP = c.CoutP; pd.CiP = c.CiP;
    const size_t pack_floats = d.dir == 0 ? (size_t)pd.ntaps * c.CinT * c.CoutP : (size_t)pd.ntaps * c.Cout * c.CiP;
    pd.tf_off = d.dir == 0 ? 0 : -1;
    pd.td_off = d.dir == 0 ? -1 : 0;
    // (+ 64 K floats: a plan whose channel splits cover more columns than the pack row holds reads past it, as inside the engine's arena,
    // where other layers' weights follow.  They hold 4096.0f here, not zeros: a read past the pack that reached a stored output would
    // show in the result)
    float* pack = (float*)sc.take((pack_floats + 65536) * 4, 0);
    PackDesc* pd_dev = (PackDesc*)sc.take(sizeof(PackDesc), 0);
    if (!pack || !pd_dev) { set_error("test_conv: out of device memory"); return OCL_ERR_HIP; }
    OCL_HIP(hipMemsetD32Async((hipDeviceptr_t)(pack + pack_floats), 0x45800000, 65536, s));
    OCL_HIP(hipMemcpyAsync(pd_dev, &pd, sizeof(pd), hipMemcpyHostToDevice, s));
    if ((rc = launch_pack_weights(o->w, pack, pd_dev, 1, c.Cout * c.Cin * pd.ntaps, s, d.dir == 0 ? PACK_TF : PACK_TD)) != OCL_OK) return rc;
    for (size_t i = 0; i < gs.size(); ++i) {
        ConvPlan p;
        if ((rc = plan_conv(gs[i], &p)) != OCL_OK) return rc;
        if ((int)i < cap && forms) test_conv_form(p, &forms[i]);
        if ((rc = conv_plan_finalize(&p, nullptr, s)) != OCL_OK) {
            conv_plan_release(&p);
            return rc;
        }
        ConvPlan q = p;
        ConvArgs& a = q.a;
        a.in = o->in; a.wT = pack; a.out = o->out; a.flags = o->flags;
        a.scale = o->scale; a.shift = o->shift; a.res = o->res; a.resmask = o->resmask;
        a.stats = (StatCell*)o->stats;
        a.stat_rep_stride = (int64_t)gs[i].groups * 2 * (d.dir == 0 ? c.Cout : c.Cin);
        if (o->xf) {
            a.xf = 1;
            a.xf_stats = (const StatCell*)o->xf_stats;
            a.xf_rep_stride = (int64_t)d.groups * 2 * c.Cin;
            a.xf_m_per_group = (int64_t)(d.n / d.groups) * c.Hin * c.Win;
            a.xf_gamma = o->xf_gamma; a.xf_beta = o->xf_beta;
            a.xf_save_mean = o->xf_save_mean; a.xf_save_invstd = o->xf_save_invstd;
            a.xf_running_mean = o->xf_running_mean; a.xf_running_var = o->xf_running_var; a.xf_nbt = o->xf_nbt;
            a.xf_momentum = 0.1f; a.xf_eps = 1e-5f;
        }
        if (o->flags & EPI_BNB) {
            if (a.bnb_lds < 0) {
                conv_plan_release(&p);
                set_error("test_conv: plan has no room for the BatchNorm-backward epilogue");
                return OCL_ERR_STATE;
            }
            a.bnb_y = o->bnb_y; a.bnb_z = o->bnb_z; a.bnb_mean = o->bnb_mean; a.bnb_invstd = o->bnb_invstd;
            a.bnb_gamma = o->bnb_gamma; a.bnb_beta = o->bnb_beta;
        }
        rc = launch_conv(q, s);
        if (rc == OCL_OK && hipStreamSynchronize(s) != hipSuccess) rc = OCL_ERR_HIP;
        conv_plan_release(&p);
        if (rc != OCL_OK) return rc;
    }
    return (int)gs.size();
}

int ocl_test_wgrad(const ocl_test_wgrad_desc* descs, const ocl_test_wgrad_ops* ops, int n_layers, int multi, int accumulate,
                   ocl_test_wgrad_form* forms, void* stream) {
    OCL_REQUIRE(descs && n_layers >= 1 && n_layers <= kMaxReduceLayers && n_layers <= kMaxWgradMulti, "test_wgrad: %d layers", n_layers);
    std::vector<WgradPlan> plans((size_t)n_layers);
    for (int i = 0; i < n_layers; ++i) {
        int rc = wgrad_plan_of(descs[i], &plans[i]);
        if (rc != OCL_OK) return rc;
        if (forms) test_wgrad_form(plans[i], &forms[i]);
    }
    if (!ops) return OCL_OK;
    int rc = conv_kernels_init();
    if (rc != OCL_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    Scratch sc;
    sc.s = s;
    // every layer's slabs side by side; all bits set (NaN): a slab row the kernel fails to write poisons the reduction
    std::vector<int64_t> off((size_t)n_layers);
    int64_t total = 0;
    for (int i = 0; i < n_layers; ++i) {
        off[i] = total;
        total += ((int64_t)plans[i].partial_floats + 63) / 64 * 64;
    }
    float* partial = (float*)sc.take((size_t)total * 4, 0xff);
    if (!partial) { set_error("test_wgrad: out of device memory"); return OCL_ERR_HIP; }
    for (int i = 0; i < n_layers; ++i) {
        const ocl_test_wgrad_ops& o = ops[i];
        OCL_REQUIRE(o.x && o.dy && o.grad, "test_wgrad: null pointer (layer %d)", i);
        WgradArgs& a = plans[i].a;
        a.x = o.x; a.dy = o.dy; a.partial = partial + off[i];
        if (o.xf) {
            OCL_REQUIRE(descs[i].xf_groups > 0 && o.xf_mean && o.xf_invstd && o.xf_gamma && o.xf_beta, "test_wgrad: input transform without operands");
            a.xf = 1; a.xf_groups = descs[i].xf_groups; a.xf_group_size = descs[i].n / descs[i].xf_groups;
            a.xf_mean = o.xf_mean; a.xf_invstd = o.xf_invstd; a.xf_gamma = o.xf_gamma; a.xf_beta = o.xf_beta;
        }
    }
    if (!multi) {
        for (int i = 0; i < n_layers; ++i) {
            if ((rc = launch_wgrad(plans[i], s)) != OCL_OK) return rc;
            if ((rc = launch_wgrad_reduce(plans[i], ops[i].grad, accumulate, s)) != OCL_OK) return rc;
        }
    } else {
        WgradMultiTable t;
        rc = launch_wgrad_multi(plans.data(), n_layers, &t, s);
        WgradReduceMulti m;
        memset(&m, 0, sizeof(m));
        m.partial = partial;
        m.grads = ops[0].grad;
        m.accumulate = accumulate;
        m.n = n_layers;
        for (int i = 0; i < n_layers; ++i) {
            OCL_REQUIRE(ops[i].grad >= ops[0].grad, "test_wgrad: multi wants the layers' gradients in one array, the first layer's first");
            wgrad_reduce_layer(plans[i], off[i], ops[i].grad - ops[0].grad, &m.L[i]);
        }
        if (rc == OCL_OK) rc = launch_wgrad_reduce_multi(m, s);
        (void)hipStreamSynchronize(s);
        wgrad_multi_release(&t);
        if (rc != OCL_OK) return rc;
    }
    OCL_HIP(hipStreamSynchronize(s));
    return OCL_OK;
}

int ocl_test_bn_fwd(const ocl_test_bn_fwd_args* t, void* stream) {
    OCL_REQUIRE(t && t->y && t->z && t->stats && t->gamma && t->beta && t->save_mean && t->save_invstd, "test_bn_fwd: null pointer");
    OCL_REQUIRE(t->groups >= 1 && t->c % 4 == 0 && t->m_per_group > 0, "test_bn_fwd: bad sizes");
    int rc = conv_kernels_init();
    if (rc != OCL_OK) return rc;
    BnFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.y = t->y; a.z = t->z; a.res = t->res; a.stats = (const StatCell*)t->stats; a.stat_rep_stride = (int64_t)t->groups * 2 * t->c;
    a.gamma = t->gamma; a.beta = t->beta; a.running_mean = t->running_mean; a.running_var = t->running_var; a.nbt = t->nbt;
    a.save_mean = t->save_mean; a.save_invstd = t->save_invstd;
    a.m_per_group = t->m_per_group; a.G = t->groups; a.C = t->c; a.relu = t->relu; a.momentum = t->momentum; a.eps = t->eps;
    a.frozen_mean = t->frozen_mean; a.frozen_var = t->frozen_var;
    a.yb = t->yb; a.stats_b = (const StatCell*)t->stats_b; a.gamma_b = t->gamma_b; a.beta_b = t->beta_b;
    a.running_mean_b = t->running_mean_b; a.running_var_b = t->running_var_b; a.nbt_b = t->nbt_b;
    a.save_mean_b = t->save_mean_b; a.save_invstd_b = t->save_invstd_b; a.frozen_mean_b = t->frozen_mean_b; a.frozen_var_b = t->frozen_var_b;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = launch_bn_fwd(a, s)) != OCL_OK) return rc;
    OCL_HIP(hipStreamSynchronize(s));
    return OCL_OK;
}

int ocl_test_bn_bwd(const ocl_test_bn_bwd_args* t, void* stream) {
    OCL_REQUIRE(t && t->dz && (t->nsets == 1 || t->nsets == 2) && t->groups >= 1 && t->c % 4 == 0 && t->m_per_group > 0, "test_bn_bwd: bad arguments");
    for (int k = 0; k < t->nsets; ++k)
        OCL_REQUIRE(t->y[k] && t->mean[k] && t->invstd[k] && t->gamma[k] && t->dy[k] && t->dgamma[k] && t->dbeta[k], "test_bn_bwd: null pointer (set %d)", k);
    OCL_REQUIRE(!t->mask_from_y || (t->nsets == 1 && !t->z && t->beta[0]), "test_bn_bwd: mask_from_y wants one set, no z, beta");
    int rc = conv_kernels_init();
    if (rc != OCL_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    Scratch sc;
    sc.s = s;
    BnBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.dz = t->dz; a.z = t->z; a.m_per_group = t->m_per_group; a.G = t->groups; a.C = t->c; a.nsets = t->nsets;
    for (int k = 0; k < 2; ++k) {
        a.y[k] = t->y[k]; a.mean[k] = t->mean[k]; a.invstd[k] = t->invstd[k]; a.gamma[k] = t->gamma[k]; a.beta[k] = t->beta[k];
        a.dy[k] = t->dy[k]; a.dgamma[k] = t->dgamma[k]; a.dbeta[k] = t->dbeta[k];
    }
    a.accumulate = t->accumulate; a.frozen = t->frozen; a.mask_from_y = t->mask_from_y;
    const size_t cells = (size_t)t->nsets * t->groups * 2 * t->c;
    a.sums = (StatCell*)sc.take(cells * sizeof(StatCell), 0);
    if (t->one_pass) {   // the engine's arena of one BatchNorm: 8 replicas x 2 groups x 2 x C cells, the arrival counters behind them
        const size_t fcells = (size_t)8 * 2 * 2 * t->c;
        a.fsums = (StatCell*)sc.take((fcells + 8) * sizeof(StatCell), 0);
        if (a.fsums) a.barrier = (unsigned*)(a.fsums + fcells);
        if (t->nsets == 2) a.fsums_b = (StatCell*)sc.take((fcells + 8) * sizeof(StatCell), 0);
    }
    if (!a.sums || (t->one_pass && (!a.fsums || !a.barrier || (t->nsets == 2 && !a.fsums_b)))) {
        set_error("test_bn_bwd: out of device memory");
        return OCL_ERR_HIP;
    }
    if ((rc = launch_bn_bwd(a, s)) != OCL_OK) return rc;
    OCL_HIP(hipStreamSynchronize(s));
    return bn_bwd_last_path();
}

int ocl_test_bn_apply_e(const float* d, const float* y, const float* mean, const float* invstd, const float* gamma, const void* esums,
                        int64_t m_per_group, int groups, int c, float* dy, float* dgamma, float* dbeta, int accumulate, void* stream) {
    OCL_REQUIRE(d && y && mean && invstd && gamma && esums && dy && dgamma && dbeta, "test_bn_apply_e: null pointer");
    int rc = conv_kernels_init();
    if (rc != OCL_OK) return rc;
    BnApplyEArgs a;
    memset(&a, 0, sizeof(a));
    a.d = d; a.y = y; a.mean = mean; a.invstd = invstd; a.gamma = gamma; a.dy = dy; a.dgamma = dgamma; a.dbeta = dbeta;
    a.esums = (const StatCell*)esums; a.esums_rep_stride = (int64_t)groups * 2 * c;
    a.m_per_group = m_per_group; a.G = groups; a.C = c; a.accumulate = accumulate;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = launch_bn_apply_e(a, s)) != OCL_OK) return rc;
    OCL_HIP(hipStreamSynchronize(s));
    return OCL_OK;
}

int ocl_test_aux(int op, const ocl_test_aux_args* t, void* stream) {
    OCL_REQUIRE(t, "test_aux: null arguments");
    int rc = conv_kernels_init();
    if (rc != OCL_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    Scratch sc;
    sc.s = s;
    const void* const* p = t->p;
    const int64_t* i = t->i;
    auto F = [&](int k) { return (float*)p[k]; };
    auto need = [&](int cnt) {
        for (int k = 0; k < cnt; ++k)
            if (!p[k]) return false;
        return true;
    };
    switch (op) {
        case OCL_AUX_LAYOUT: {
            OCL_REQUIRE(need(3) && i[0] >= 1 && i[0] <= kMaxInputSegments && i[1] > 0 && i[2] > 0, "test_aux: layout arguments");
            const float* const* xs = (const float* const*)p[0];
            const int32_t* ns = (const int32_t*)p[1];
            InputSegments sg;
            memset(&sg, 0, sizeof(sg));
            sg.n = (int)i[0];
            int N = 0;
            for (int k = 0; k < sg.n; ++k) {
                OCL_REQUIRE(xs[k] && ns[k] > 0, "test_aux: layout segment %d", k);
                sg.x[k] = xs[k];
                sg.first[k] = N;
                N += ns[k];
            }
            rc = launch_nchw3_to_nhwc4_segments(sg, F(2), N, (int)i[1], (int)i[2], s);
            break;
        }
        case OCL_AUX_AVGPOOL_FWD:
        case OCL_AUX_AVGPOOL_BWD:
            OCL_REQUIRE(need(2) && i[0] > 0 && i[1] >= 4 && i[2] >= 4 && i[3] > 0, "test_aux: avgpool arguments");
            rc = op == OCL_AUX_AVGPOOL_FWD ? launch_avgpool_fwd(F(0), F(1), (int)i[0], (int)i[1], (int)i[2], (int)i[3], s)
                                           : launch_avgpool_bwd(F(0), F(1), (int)i[0], (int)i[1], (int)i[2], (int)i[3], s);
            break;
        case OCL_AUX_L2NORM_FWD:
            OCL_REQUIRE(need(3) && i[0] > 0 && i[1] > 0, "test_aux: l2norm arguments");
            rc = launch_l2norm_fwd(F(0), F(1), F(2), (int)i[0], (int)i[1], s, F(3));
            break;
        case OCL_AUX_L2NORM_BWD:
            OCL_REQUIRE(need(4) && i[0] > 0 && i[1] > 0, "test_aux: l2norm arguments");
            rc = launch_l2norm_bwd(F(0), F(1), F(2), F(3), (int)i[0], (int)i[1], s);
            break;
        case OCL_AUX_RELU_BWD:
            OCL_REQUIRE(need(3) && i[0] > 0, "test_aux: relu_bwd arguments");
            rc = launch_relu_bwd(F(0), F(1), F(2), i[0], s);
            break;
        case OCL_AUX_COLSUM:
            OCL_REQUIRE(need(2) && i[0] > 0 && i[1] > 0, "test_aux: colsum arguments");
            rc = launch_colsum(F(0), (int)i[0], (int)i[1], F(1), (int)i[2], s);
            break;
        case OCL_AUX_FILL:
            OCL_REQUIRE(need(1) && i[0] >= 0, "test_aux: fill arguments");
            rc = launch_fill(F(0), i[0], t->f[0], s);
            break;
        case OCL_AUX_BN_FOLD: {
            OCL_REQUIRE(need(3), "test_aux: bn_fold arguments");
            NetTestTables nt;
            if ((rc = net_test_tables((int)i[0], (int)i[1], &nt)) != OCL_OK) return rc;
            const size_t bytes = nt.fold.size() * sizeof(BnFoldDesc);
            BnFoldDesc* dev = (BnFoldDesc*)sc.take(bytes, 0);
            if (!dev) { set_error("test_aux: out of device memory"); return OCL_ERR_HIP; }
            OCL_HIP(hipMemcpyAsync(dev, nt.fold.data(), bytes, hipMemcpyHostToDevice, s));
            rc = launch_bn_fold(F(0), F(1), F(2), dev, (int)nt.fold.size(), t->f[0], s);
            OCL_HIP(hipStreamSynchronize(s));   // (the host table goes out of scope)
            break;
        }
        case OCL_AUX_BN_APPLY_SAVED:
            OCL_REQUIRE(need(6) && i[0] > 0 && i[1] > 0 && i[2] > 0 && i[2] % 4 == 0, "test_aux: bn_apply_saved arguments");
            rc = launch_bn_apply_saved(F(0), F(1), F(2), F(3), F(4), F(5), i[0], (int)i[1], (int)i[2], s);
            break;
        default:
            set_error("test_aux: op=%d", op);
            return OCL_ERR_ARG;
    }
    if (rc != OCL_OK) return rc;
    OCL_HIP(hipStreamSynchronize(s));
    return OCL_OK;
}

int ocl_test_pack_all(int hw, int nf, int mask, const float* params, float* arena, void* zero_a, int64_t zero_a_cells, void* zero_b,
                      int64_t zero_b_cells, int64_t* table, int table_cap, int64_t* sizes, void* stream) {
    OCL_REQUIRE(mask >= 1 && mask <= PACK_ALL && zero_a_cells >= 0 && zero_b_cells >= 0, "test_pack_all: mask=%d", mask);
    OCL_REQUIRE((zero_a || !zero_a_cells) && (zero_b || !zero_b_cells), "test_pack_all: cells without an array");
    NetTestTables nt;
    int rc = net_test_tables(hw, nf, &nt);
    if (rc != OCL_OK) return rc;
    const int L = (int)nt.pack.size();
    for (int l = 0; table && l < L && l < table_cap; ++l) {
        const PackDesc& d = nt.pack[l];
        const int64_t row[9] = {d.w_off, d.tf_off, d.td_off, d.Cout, d.Cin, d.ntaps, d.CinP, d.CoutP, d.CiP};
        memcpy(table + (size_t)l * 9, row, sizeof(row));
    }
    if (sizes) {
        sizes[0] = nt.n_params;
        sizes[1] = nt.pack_floats;
    }
    if (!arena) return L;
    OCL_REQUIRE(params, "test_pack_all: null params");
    if ((rc = conv_kernels_init()) != OCL_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    Scratch sc;
    sc.s = s;
    PackDesc* dev = (PackDesc*)sc.take((size_t)L * sizeof(PackDesc), 0);
    if (!dev) { set_error("test_pack_all: out of device memory"); return OCL_ERR_HIP; }
    OCL_HIP(hipMemcpyAsync(dev, nt.pack.data(), (size_t)L * sizeof(PackDesc), hipMemcpyHostToDevice, s));
    rc = launch_pack_weights(params, arena, dev, L, nt.max_elems, s, mask, (StatCell*)zero_a, zero_a_cells, (StatCell*)zero_b, zero_b_cells);
    OCL_HIP(hipStreamSynchronize(s));
    return rc == OCL_OK ? L : rc;
}

int ocl_set_deterministic(int on) { return set_deterministic_sums(on); }

}  // extern "C"
