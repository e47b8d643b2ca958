#pragma once
#include <memory>

#include "nn/expert_set.h"
#include "nn/rise_net.h"

// A net handle of the C API: a plain net (mi_net_create) or a set of game-phase experts (mi_net_create_experts).  `any` is what both
// kinds share; exactly one of `plain` / `experts` points at the same object under its own type.
struct mi_net {
    std::unique_ptr<cra::BoardNet> any;
    cra::RiseNet* plain = nullptr;
    cra::ExpertSet* experts = nullptr;
    mi_net(const char* dir, int dev, int batch, const char* prec) : plain(new cra::RiseNet(dir ? dir : "", dev, batch, prec ? prec : "float16")) { any.reset(plain); }
    mi_net(const char* dir, int dev, int batch, const char* prec, int phase_definition)
        : experts(new cra::ExpertSet(dir ? dir : "", dev, batch, prec ? prec : "float16x3", phase_definition)) { any.reset(experts); }
};
