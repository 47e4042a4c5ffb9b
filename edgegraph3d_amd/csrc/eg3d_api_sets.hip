// eg3d_api_sets.hip — polyline sets that stay on the device (include/eg3d_sets_device.h): the three producers of a device
// view (upload + device checks, K9's rows in place, K13), and the entry points of the extractor on item ranges, whose
// cutting and units live with the other calls on polyline sets in eg3d_api_match_sets.hip. Host orchestration only: the
// kernels are in eg3d_k13_sets.hip.
#include "../../include/eg3d_sets_device.h"
#include "eg3d_api_match_internal.h"
#include "eg3d_k13_sets.h"

namespace {

void fill_view(const eg3d_ctx* c, const eg3d_ctx::ResidentSets& rs, const DevBuf& off, const DevBuf& ids, eg3d_device_polyline_sets* out) {
  memset(out, 0, sizeof(*out));
  out->struct_size = (uint32_t)sizeof(*out);
  out->n_sets = rs.n_sets;
  out->n_views = c->V;
  out->device = c->device;
  out->n_ids = rs.n_ids;
  out->row_off = off.as<uint32_t>();
  out->pl_ids = ids.as<uint32_t>();
}

// A view is accepted by the context whose buffers it points into, while what it says is still what those buffers hold.
int open_view(eg3d_ctx* c, const char* who, const eg3d_device_polyline_sets* v, SetsDev* sd, uint32_t* n_rows) {
  if (!c || !v) {
    g_err = std::string(who) + ": bad arguments";
    return EG3D_ERR_ARG;
  }
  BUF_TRY(check_struct_size(who, "eg3d_device_polyline_sets", v->struct_size, sizeof(eg3d_device_polyline_sets), "sets"));
  const struct {
    const eg3d_ctx::ResidentSets* rs;
    const DevBuf* off;
    const DevBuf* ids;
  } producers[3] = {{&c->rs_upload, &c->u_sets_off, &c->u_sets_ids}, {&c->rs_k9, &c->k9_rowoff, &c->k9_plids}, {&c->rs_k13, &c->k13_rowoff, &c->k13_plids}};
  for (const auto& p : producers)
    if (p.rs->valid && v->row_off && v->row_off == p.off->as<uint32_t>() && v->pl_ids == p.ids->as<uint32_t>() && v->n_sets == p.rs->n_sets &&
        v->n_ids == p.rs->n_ids && v->n_views == c->V && v->device == c->device) {
      sd->n_views = (uint32_t)c->V;
      sd->row_off = v->row_off;
      sd->pl_ids = v->pl_ids;
      *n_rows = v->n_sets * (uint32_t)c->V;
      return EG3D_OK;
    }
  g_err = std::string(who) + ": the sets are not a current device view of this context (include/eg3d_sets_device.h: what ends a view)";
  return EG3D_ERR_ARG;
}

}  // namespace

extern "C" int eg3d_upload_polyline_sets(eg3d_ctx* c, const eg3d_polyline_sets* ps, eg3d_device_polyline_sets* out) {
  if (!c || !ps || !out || !ps->row_off) {
    g_err = "eg3d_upload_polyline_sets: bad arguments";
    return EG3D_ERR_ARG;
  }
  const uint32_t V = (uint32_t)c->V;
  if ((uint64_t)ps->n_sets * V >= 0xffffffffull) {
    g_err = "eg3d_match_polyline_sets: too many rows";
    return EG3D_ERR_ARG;
  }
  const uint32_t n_rows = ps->n_sets * V;
  const uint32_t n_ids = ps->row_off[n_rows];  // (sizes the upload; the device check below holds every offset to it)
  if (n_ids && !ps->pl_ids) {
    g_err = "eg3d_match_polyline_sets: pl_ids is null";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  c->rs_upload.valid = false;
  BUF_TRY(upload(c->u_sets_off, ps->row_off, (size_t)n_rows + 1, st));
  BUF_TRY(upload(c->u_sets_ids, ps->pl_ids, n_ids, st));
  BUF_TRY(c->u_bad.ensure(sizeof(uint32_t)));
  HIP_TRY(hipMemsetAsync(c->u_bad.p, 0, sizeof(uint32_t), st));
  SetsDev sd;
  sd.n_views = V;
  sd.row_off = c->u_sets_off.as<uint32_t>();
  sd.pl_ids = c->u_sets_ids.as<uint32_t>();
  launch_k13_check_sets(st, c->ds, sd, n_rows, n_ids, c->u_bad.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  uint32_t bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, c->u_bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // (also: the caller's pageable arrays have been read)
  if (bad) {
    g_err = bad & K13_SETS_BAD_START    ? "eg3d_upload_polyline_sets: row_off does not begin at 0"
            : bad & K13_SETS_BAD_ORDER  ? "eg3d_match_polyline_sets: row_off is not ascending"
            : bad & K13_SETS_BAD_RANGE  ? "eg3d_match_polyline_sets: polyline id out of range"
                                        : "eg3d_match_polyline_sets: polyline ids of a row are not strictly ascending";
    return EG3D_ERR_ARG;
  }
  c->rs_upload.valid = true;
  c->rs_upload.n_sets = ps->n_sets;
  c->rs_upload.n_ids = n_ids;
  fill_view(c, c->rs_upload, c->u_sets_off, c->u_sets_ids, out);
  return EG3D_OK;
}

extern "C" int eg3d_polyline_matches_device(eg3d_ctx* c, eg3d_device_polyline_sets* out) {
  if (!c || !out) {
    g_err = "eg3d_polyline_matches_device: bad arguments";
    return EG3D_ERR_ARG;
  }
  if (!c->rs_k9.valid) {
    g_err = "eg3d_polyline_matches_device: no eg3d_match_polylines_closeness call has completed on this context";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  if (!c->rs_k9.n_ids) {  // (a call that matched nothing wrote no row: the view is n_sets * V + 1 zero offsets)
    BUF_TRY(c->k9_rowoff.ensure(sizeof(uint32_t) * ((size_t)c->rs_k9.n_sets * (uint32_t)c->V + 1)));
    BUF_TRY(c->k9_plids.ensure(sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(c->k9_rowoff.p, 0, sizeof(uint32_t) * ((size_t)c->rs_k9.n_sets * (uint32_t)c->V + 1), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  fill_view(c, c->rs_k9, c->k9_rowoff, c->k9_plids, out);
  return EG3D_OK;
}

extern "C" int eg3d_sets_from_communities_device(eg3d_ctx* c, const int64_t* ids_host, uint64_t n, eg3d_device_polyline_sets* out,
                                                 eg3d_sets_device_stats* stats) {
  static const char who[] = "eg3d_sets_from_communities_device";
  if (stats) BUF_TRY(check_struct_size(who, "eg3d_sets_device_stats", stats->struct_size, sizeof(eg3d_sets_device_stats)));
  if (!c || !out) {
    g_err = std::string(who) + ": bad arguments";
    return EG3D_ERR_ARG;
  }
  if (!c->k10_valid) {
    g_err = std::string(who) + ": no eg3d_similarity_graph call has completed on this context: there are no nodes";
    return EG3D_ERR_ARG;
  }
  if (n != c->k10_nodes) {
    g_err = std::string(who) + ": n is not the n_nodes of the last eg3d_similarity_graph call on this context";
    return EG3D_ERR_ARG;
  }
  if (!ids_host && (!c->k11_valid || c->k11_nodes != c->k10_nodes)) {
    g_err = std::string(who) + ": ids_host is NULL and no eg3d_detect_communities call on this graph's nodes has completed on this context";
    return EG3D_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  BUF_TRY(ensure_mailbox(c));
  c->rs_k13.valid = false;
  const uint32_t nn = (uint32_t)n, V = (uint32_t)c->V;
  float ms_upload = 0, ms_device = 0;
  const int64_t* ids = c->k11[K11B_IDS].as<int64_t>();
  if (ids_host) {
    const auto t0 = std::chrono::steady_clock::now();
    BUF_TRY(upload(c->k13_ids, ids_host, nn, st));
    HIP_TRY(hipStreamSynchronize(st));  // (the caller's pageable array)
    ms_upload = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ids = c->k13_ids.as<int64_t>();
  }
  const uint32_t* node_view = c->k10_nodeview.as<uint32_t>();
  const uint32_t* node_pl = c->k10_nodepl.as<uint32_t>();
  BUF_TRY(c->k13_flag.ensure(sizeof(uint32_t) * ((size_t)nn + 1)));
  BUF_TRY(c->k13_pos.ensure(sizeof(uint32_t) * ((size_t)nn + 1)));
  for (int k = 0; k < 2; k++) BUF_TRY(c->k13_key[k].ensure(8 * std::max<size_t>(nn, 1)));
  BUF_TRY(c->k13_ctr.ensure(4 * sizeof(unsigned long long)));  // [0] max id + 1, [1] flag word, [2] distinct keys (32 bits)
  unsigned long long* ctr = c->k13_ctr.as<unsigned long long>();
  uint32_t* named = c->k13_flag.as<uint32_t>();
  uint32_t* pos = c->k13_pos.as<uint32_t>();
  unsigned long long* key[2] = {c->k13_key[0].as<unsigned long long>(), c->k13_key[1].as<unsigned long long>()};
  HIP_TRY(hipEventRecord(c->ea[0], st));
  HIP_TRY(hipMemsetAsync(ctr, 0, 4 * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(named + nn, 0, sizeof(uint32_t), st));
  // ---- (1) validate, and how many sets and named nodes there are
  launch_k13_validate(st, ids, node_view, node_pl, nn, V, named, ctr);
  HIP_TRY(hipGetLastError());
  BUF_TRY(scan_u32(c, named, pos, (size_t)nn + 1));
  uint64_t n_sets = 0;
  uint32_t n_named = 0, n_ids = 0;
  {
    Readback rb(c);
    const int ic = rb.add(ctr, 4);
    const int it = rb.add(pos + nn, 1);
    BUF_TRY(rb.run());
    n_sets = (uint64_t)rb.item(ic)[0] | ((uint64_t)rb.item(ic)[1] << 32);
    const uint32_t bad = rb.item(ic)[2];
    n_named = *rb.item(it);
    if (n_sets * (uint64_t)V >= 0xffffffffull) {  // (the host statement's order: capacity first)
      g_err = std::string(who) + ": the result has more than 2^32-2 rows (sets x views)";
      return EG3D_ERR_CAPACITY;
    }
    if (bad) {
      g_err = std::string(who) + (bad & K13_BAD_VIEW ? ": a node of a community lies in a view the scene does not have"
                                                     : ": a node's polyline id is 2^19 or more");
      return EG3D_ERR_ARG;
    }
  }
  const uint32_t n_rows = (uint32_t)n_sets * V;
  // ---- (2) .. (4) the keys behind the scan, sorted, equal neighbours dropped
  if (n_named) {
    launch_k13_keys(st, ids, node_view, node_pl, nn, V, named, pos, key[0]);
    HIP_TRY(hipGetLastError());
    BUF_TRY(sort_keys_u64(c, key[0], key[1], n_named));
    BUF_TRY(unique_u64(c, key[1], key[0], (uint32_t*)(ctr + 2), n_named));
    Readback rb(c);
    const int iu = rb.add(ctr + 2, 1);
    BUF_TRY(rb.run());
    n_ids = *rb.item(iu);
  }
  // ---- (5) the offsets, as K9's tail
  BUF_TRY(c->k13_rowoff.ensure(sizeof(uint32_t) * ((size_t)n_rows + 1)));
  BUF_TRY(c->k13_plids.ensure(sizeof(uint32_t) * std::max<size_t>(n_ids, 1)));
  if (n_ids)
    launch_k0_csr(st, key[0], n_ids, n_rows, c->k13_rowoff.as<uint32_t>(), c->k13_plids.as<uint32_t>());
  else
    HIP_TRY(hipMemsetAsync(c->k13_rowoff.p, 0, sizeof(uint32_t) * ((size_t)n_rows + 1), st));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->eb[0], st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipEventElapsedTime(&ms_device, c->ea[0], c->eb[0]));
  c->rs_k13.valid = true;
  c->rs_k13.n_sets = (uint32_t)n_sets;
  c->rs_k13.n_ids = n_ids;
  fill_view(c, c->rs_k13, c->k13_rowoff, c->k13_plids, out);
  if (stats) {
    stats->struct_size = (uint32_t)sizeof(eg3d_sets_device_stats);
    stats->n_nodes = nn;
    stats->n_named = n_named;
    stats->n_sets = (uint32_t)n_sets;
    stats->n_ids = n_ids;
    stats->ms_device = ms_device;
    stats->ms_upload = ms_upload;
  }
  return EG3D_OK;
}

extern "C" int eg3d_polyline_item_samples(eg3d_ctx* c, const eg3d_device_polyline_sets* sets, uint32_t item_begin, uint32_t item_end,
                                          const eg3d_matched_intervals* m, uint32_t* counts_host) {
  static const char who[] = "eg3d_polyline_item_samples";
  SetsDev sd;
  uint32_t n_rows = 0;
  BUF_TRY(open_view(c, who, sets, &sd, &n_rows));
  if (item_begin > item_end || item_end > sets->n_ids || (item_end > item_begin && !counts_host)) {
    g_err = std::string(who) + ": bad arguments (the item range lies outside the sets, or counts_host is NULL)";
    return EG3D_ERR_ARG;
  }
  return count_item_samples(c, sd, n_rows, item_begin, item_end, m, counts_host, nullptr);
}

extern "C" int eg3d_match_polyline_items(eg3d_ctx* c, const eg3d_device_polyline_sets* sets, const eg3d_items_call* call,
                                         const eg3d_matched_intervals* m, int device_only, eg3d_edgepoints* out,
                                         eg3d_stage_times* times) {
  static const char who[] = "eg3d_match_polyline_items";
  SetsDev sd;
  uint32_t n_rows = 0;
  BUF_TRY(open_view(c, who, sets, &sd, &n_rows));
  if (!call || !out) {
    g_err = std::string(who) + ": bad arguments";
    return EG3D_ERR_ARG;
  }
  BUF_TRY(check_struct_size(who, "eg3d_items_call", call->struct_size, sizeof(eg3d_items_call), "call"));
  if (call->item_begin > call->item_end || call->item_end > sets->n_ids) {
    g_err = std::string(who) + ": the item range lies outside the sets";
    return EG3D_ERR_ARG;
  }
  return match_items_call(c, sd, n_rows, call->item_begin, call->item_end, call->sample_base, m, device_only, out, times);
}

extern "C" int eg3d_polyline_items_units(eg3d_ctx* c, uint32_t* n_units, uint32_t* n_redone) {
  if (!c || !n_units || !n_redone) {
    g_err = "eg3d_polyline_items_units: bad arguments";
    return EG3D_ERR_ARG;
  }
  *n_units = c->items_units;
  *n_redone = c->items_redone;
  return EG3D_OK;
}
