// k_dqr_sample's body, block-wide (256 threads), as text: included by k_dqr_sample and by k_dqp_sample
// (pm_dqn_replay.hip), with d (pm_dqn), rp (pm_dqn_replay), upd (int) and sm (DqrSampleSmem, LDS) in scope.
// It is shared as text, not as a __device__ function, because k_dqr_sample must keep its device text: routed
// through a function the compiler schedules seven instructions of the weights' maximum in another order
// (tools/kernel_text.py: DIFFER), whichever way the descriptors are handed over. k_dqr_scatter's body, which
// does keep its text behind a function, is one (dqr_scatter_body). PM_DQR_HORIZON(j, bits) is the including kernel's
// own: nothing in k_dqr_sample / k_dqp_sample, the store of row j's horizon byte in their _n forms.
    const int t = threadIdx.x, wv = t >> 6, B = d.batch;
    const int64_t frame = d.stats->steps + 1;  // frame_idx += 1 before sampling (:136)
    const double b = rp.beta_start + (double)frame * (1.0 - rp.beta_start) / (double)rp.beta_frames;  // :137
    const double beta = b < 1.0 ? b : 1.0;
    const PerTree tr = per_tree(rp.per_work, rp.cap);
    const double* u = rp.u ? rp.u + (size_t)upd * B : nullptr;
    int bad = 0;
    for (int j0 = 0; j0 < B; j0 += PER_BS)
        per_sample_block<true>(
            true, rp.size, tr, PushRange{0, 0, rp.cap, 0.f}, beta, j0, B, sm.per,
            [&](int j) {
                if (u) return u[j];
                const U4 r = philox64((uint32_t)j, TAG_PER, (uint64_t)frame, rp.seed);
                return u53(r.x, r.y);
            },
            [&](int j, int64_t i, double pa, double total) {
                sm.sidx[j] = i;
                sm.w[j] = per_is_weight(rp.size, pa, total, beta);
                if (!(total > 0.0)) bad |= DQR_NO_MASS;
                else if (i < 0 || i >= rp.size) bad |= DQR_BAD_SLOT;
            });
    const int no_mass = __syncthreads_or(bad & DQR_NO_MASS), bad_slot = __syncthreads_or(bad & DQR_BAD_SLOT);
    if (no_mass || bad_slot) {  // block-uniform: a void update
        if (t < B) rp.idx[t] = -1;
        if (t == 0) atomicOr(&d.stats->status, (no_mass ? DQR_NO_MASS : 0) | (bad_slot ? DQR_BAD_SLOT : 0));
        return;
    }
    {
        const float m = wave_max(t < B ? sm.w[t] : 0.f);
        if ((t & 63) == 0) sm.red[wv] = m;
    }
    __syncthreads();
    const float mx = fmaxf(fmaxf(sm.red[0], sm.red[1]), fmaxf(sm.red[2], sm.red[3]));
    // the batch buffers are the learner's own: pm_dqn declares them const for the entry points that only read them
    float* const s = const_cast<float*>(d.s);
    float* const ns = const_cast<float*>(d.ns);
    float* const rew = const_cast<float*>(d.rew);
    float* const isw = const_cast<float*>(d.isw);
    int32_t* const act = const_cast<int32_t*>(d.act);
    uint8_t* const done = const_cast<uint8_t*>(d.done);
    const int q = t & 3;
    for (int j = t >> 2; j < B; j += PER_BS) {
        const int64_t i = sm.sidx[j];  // in [0, size): checked above
        const float4 x = reinterpret_cast<const float4*>(rp.trans + i * PM_TRANS_F)[q];
        float* const o = (q < 2 ? s : ns) + (size_t)j * 7 + 4 * (q & 1);
        o[0] = x.x; o[1] = x.y; o[2] = x.z;
        if (q == 0) {
            o[3] = x.w;
            rp.idx[j] = i;
            isw[j] = sm.w[j] / mx;  // k_per_normalize's division
        } else if (q == 1) {
            rew[j] = x.w;
        } else if (q == 2) {
            o[3] = x.w;
        } else {
            const int bits = __float_as_int(x.w);
            act[j] = bits & 0xff;
            done[j] = (uint8_t)((bits >> 8) & 1);
            PM_DQR_HORIZON(j, bits);
        }
    }
