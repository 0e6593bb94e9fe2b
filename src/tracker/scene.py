from .. import _pkg

SceneWatch = _pkg("scene").SceneWatch
