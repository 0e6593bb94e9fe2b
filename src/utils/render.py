from .. import _pkg

Renderer = _pkg("render").Renderer
