// kp_explain.h — operands and rows of explain_kernel (kp_explain.hip), shared with the host (kp_host.cpp
// kp_solve_explain).  Plain data, as kp_layout.h.
//
// Scheduler.Solve ends after a full queue cycle without a placement, so every pod it leaves unschedulable made its last
// add() against the state the Solve ended in.  Core's error for such a pod lists one failure per NodeClaimTemplate of
// that add(); explain_kernel recomputes it from the final state the Solve kernels leave in HBM (remaining limits,
// template options, topology counts, the pods' final relaxation stage), read-only, one wave per
// (distinct unschedulable shape, template).  DESIGN.md §4 "Explanations".
#pragma once
#include <stdint.h>

// One (shape, template) diagnosis.  reason is a KP_WHY_* of include/kpsim.h (the host asserts the two enumerations
// agree).  kmask names every failing key, so the host can pick the one whose name sorts first: for KPX_REQUIREMENTS
// bit i is class key i of the shape's class (KpDev.cls_keys), for KPX_MIN_VALUES entry i of the template's min_keys row.
struct KpExplainRow {
    int32_t reason;
    uint32_t kmask;
    uint32_t criteria;       // filterResults' six flags, KPX_C_*
    int32_t n_options;       // template options within the NodePool's remaining limits
    int32_t n_requirements;  // of those: compatible with the merged requirements / fitting the requests / with a
    int32_t n_fits;          // compatible available offering (0 when an earlier stage failed)
    int32_t n_offering;
    int32_t hostkey;         // KPX_REQUIREMENTS: the class's hostname requirement fails as well (KpExplain.hblock)
};

enum { KPX_UNKNOWN = 0, KPX_LIMITS, KPX_TAINTS, KPX_HOST_PORTS, KPX_REQUIREMENTS, KPX_TOPOLOGY, KPX_INSTANCE_TYPES,
       KPX_MIN_VALUES, KPX_RESERVED };
enum { KPX_C_REQ = 1u, KPX_C_FITS = 2u, KPX_C_OFF = 4u, KPX_C_REQ_FITS = 8u, KPX_C_REQ_OFF = 16u, KPX_C_FITS_OFF = 32u };

struct KpExplain {
    const int32_t* rep;      // [n_shapes] a pod of each distinct shape (its pod_cls / pod_req rows are the shape's)
    int32_t n_shapes;
    int32_t pad;
    uint64_t born;           // late topology identities the Solve created (KpDev.tg_late), for variant routing
    // KpDev.tol folds two things into one mask: the tolerations, and a hostname requirement no NodeClaim's placeholder
    // can satisfy (In, DoesNotExist, Gt, Lt: such a class has every bit clear and no hostname class key).  A diagnosis
    // needs them apart: core reports the second as incompatible requirements on kubernetes.io/hostname.
    const uint64_t* tol;     // [C] bit j: the class tolerates template j's taints
    const uint8_t* hblock;   // [C] the class's hostname requirement refuses every new NodeClaim
    KpExplainRow* rows;      // [n_shapes][NT]
};
