#pragma once
#include <memory>

#include "search/pool.h"

struct mi_search {
    std::unique_ptr<cra::search::SearchPool> pool;
    int expert_routing = 0;      // mi_search_settings::expert_routing, for the lanes added later (mi_search_add_lane)
};
