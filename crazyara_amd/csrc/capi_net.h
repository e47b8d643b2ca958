#pragma once
#include "nn/rise_net.h"

struct mi_net {
    cra::RiseNet net;
    mi_net(const char* dir, int dev, int batch, const char* prec) : net(dir ? dir : "", dev, batch, prec ? prec : "float16") {}
    mi_net(const char* dir, int dev, int batch, const char* prec, int phase_definition)      // an expert set (mi_net_create_experts)
        : net(cra::RiseNet::ExpertSet{}, dir ? dir : "", dev, batch, prec ? prec : "float16x3", phase_definition) {}
};
