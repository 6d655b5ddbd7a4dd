// rx_plan_check — prints the launch form udpdk_gpu_rx would take, on a machine without a GPU:
// rx_plan.h's planner and knob parser behind a main(), no HIP call, no project library
// (tests/test_rx_plan.py compares the output with the trace recorded on a GPU).
//
// Rows on stdin, one per line, `#` starts a comment:
//   n lanes fanout tail_recent [KEY=VAL ...]    -> classify<G>[ fused] | <form line> | <launch numbers>
//   knobs [KEY=VAL ...]                         -> the parsed RxKnobs
// KEY is an environment knob (UDPDK_...: set for this row only, then rx_knobs_from_env()), or
// max_frames / max_lanes (the context's bounds, default n and lanes) or hist_cap / partial_cap /
// tiles_cap (one capacity of rx_caps() overridden).

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "rx_plan.h"

using namespace udpdk;

static const char *const KNOB_ENV[] = {
    "UDPDK_ONE_LANE_TILE", "UDPDK_RX_HIST_CAP", "UDPDK_RX_FUSE", "UDPDK_RX_TRACE", "UDPDK_RX_NO_INLINE",
    "UDPDK_RX_SCAN_COLS_TILES", "UDPDK_RX_MR", "UDPDK_RX_SPAN", "UDPDK_RX_POLICY", "UDPDK_SCATTER_GROUP_FRAMES",
    "UDPDK_SCATTER_MIN_WG", "UDPDK_RX_TAILG", "UDPDK_TX_PARTS", "UDPDK_TX_GRID", "UDPDK_GATHER_GRID"};

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        line = line.substr(0, line.find('#'));
        std::istringstream in(line);
        std::vector<std::string> w;
        for (std::string t; in >> t;) w.push_back(t);
        if (w.empty()) continue;
        const bool knobs_row = w[0] == "knobs";
        const size_t first_kv = knobs_row ? 1 : 4;
        if (w.size() < first_kv) {
            fprintf(stderr, "rx_plan_check: bad row: %s\n", line.c_str());
            return 2;
        }
        for (const char *e : KNOB_ENV) unsetenv(e);
        unsigned long long v[4] = {};
        for (size_t i = 0; i < 4 && !knobs_row; ++i) v[i] = strtoull(w[i].c_str(), nullptr, 0);
        const uint32_t n = (uint32_t)v[0], lanes = (uint32_t)v[1], fanout = (uint32_t)v[2];
        unsigned long long max_frames = n, max_lanes = lanes, cap[3] = {};
        bool cap_set[3] = {};
        for (size_t i = first_kv; i < w.size(); ++i) {
            const size_t eq = w[i].find('=');
            if (eq == std::string::npos) {
                fprintf(stderr, "rx_plan_check: not KEY=VAL: %s\n", w[i].c_str());
                return 2;
            }
            const std::string key = w[i].substr(0, eq), val = w[i].substr(eq + 1);
            static const char *const CAPS[3] = {"hist_cap", "partial_cap", "tiles_cap"};
            if (key.rfind("UDPDK_", 0) == 0) setenv(key.c_str(), val.c_str(), 1);
            else if (key == "max_frames") max_frames = strtoull(val.c_str(), nullptr, 0);
            else if (key == "max_lanes") max_lanes = strtoull(val.c_str(), nullptr, 0);
            else {
                size_t k = 0;
                while (k < 3 && key != CAPS[k]) ++k;
                if (k == 3) {
                    fprintf(stderr, "rx_plan_check: unknown key %s\n", key.c_str());
                    return 2;
                }
                cap[k] = strtoull(val.c_str(), nullptr, 0);
                cap_set[k] = true;
            }
        }
        const RxKnobs k = rx_knobs_from_env();
        if (knobs_row) {
            printf("one_lane_tile %u geo_cap %llu force_fuse %d force_tailg %d force_mr %d no_span %d policy %d "
                   "trace %d scan_cols_tiles %u no_inline %d scatter_group_frames %u scatter_min_wg %u tx_parts %u "
                   "tx_grid %u gather_grid %u\n", k.one_lane_tile, (unsigned long long)k.geo_cap, k.force_fuse,
                   k.force_tailg, k.force_mr, (int)k.no_span, k.policy, (int)k.trace, k.scan_cols_tiles,
                   (int)k.no_inline, k.scatter_group_frames, k.scatter_min_wg, k.tx_parts, k.tx_grid, k.gather_grid);
            continue;
        }
        RxCaps caps = rx_caps((uint32_t)max_frames, (uint32_t)max_lanes, k.geo_cap);
        if (cap_set[0]) caps.hist_cap = cap[0];
        if (cap_set[1]) caps.partial_cap = cap[1];
        if (cap_set[2]) caps.tiles_cap = cap[2];
        const RxPlan p = rx_plan(n, lanes, fanout, v[3] != 0, k, caps);
        char cls[32], form[128];
        rx_plan_trace(p, cls, form);
        printf("%s | %s | lb %u scan_grid %u nc %u lds %u compact_grid %u tile_base %d span %d rc %d\n", cls, form,
               p.lb, p.scan_grid, p.nc, p.cls_lds, p.compact_grid, (int)p.tile_base, (int)p.span, p.err);
    }
    return 0;
}
